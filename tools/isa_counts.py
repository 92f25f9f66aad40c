#!/usr/bin/env python3
"""Static instruction counts and resources per kernel of gfx950 assembly files (hipcc --save-temps, as tools/isa_diff.py builds them).  CPU only.

    python tools/isa_counts.py NAME=DIR [NAME=DIR ...] [--kernels REGEX]      # DIR holds *-hip-amdgcn-*gfx950.s

Prints one JSON document {NAME: {unit:kernel: {vector, lds, lds_read_b128, lds_write_b128, dpp, mfma, accvgpr, salu, vmem, total, vgpr, accum_offset,
sgpr, scratch_bytes, lds_bytes}}}: the text between a kernel's label and its .Lfunc_end, every instruction counted once (loops are not weighted).
A kernel with workgroup barriers also gets between_barriers: [{vector, lds, total}] for the text between consecutive s_barrier instructions."""
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_diff import kernels

RES = {"vgpr": "next_free_vgpr", "accum_offset": "accum_offset", "sgpr": "next_free_sgpr", "scratch_bytes": "private_segment_fixed_size",
       "lds_bytes": "group_segment_fixed_size"}


def count(body, block):
    ops = [ln.split()[0] for ln in body if not ln.lstrip().startswith(".") and not ln.rstrip().endswith(":")]
    text = [ln for ln in body if not ln.lstrip().startswith(".") and not ln.rstrip().endswith(":")]
    c = {"vector": sum(o.startswith("v_") for o in ops), "lds": sum(o.startswith("ds_") for o in ops),
         "lds_read_b128": ops.count("ds_read_b128"), "lds_write_b128": ops.count("ds_write_b128"),
         "dpp": sum(("quad_perm" in ln or "row_" in ln or "_dpp" in ln.split()[0]) for ln in text), "mfma": sum(o.startswith("v_mfma") for o in ops),
         "accvgpr": sum(o.startswith("v_accvgpr") for o in ops), "salu": sum(o.startswith("s_") for o in ops),
         "vmem": sum(o.startswith(("global_", "buffer_", "flat_", "scratch_")) for o in ops), "total": len(ops)}
    if "s_barrier" in ops:
        # kernels with workgroup barriers (k_step_h2, k_step_h3): the instructions between consecutive barriers in text order, first and last
        # segment included.  The wavefronts' code follows one another in the text, wavefront 0's first: its second segment is what it issues
        # between the two barriers of a sub-step, and each helper's chain is the segment between that helper's pair
        cuts = [-1] + [i for i, o in enumerate(ops) if o == "s_barrier"] + [len(ops)]
        c["between_barriers"] = [{"vector": sum(o.startswith("v_") for o in ops[a + 1:b]), "lds": sum(o.startswith("ds_") for o in ops[a + 1:b]), "total": b - a - 1}
                                 for a, b in zip(cuts, cuts[1:])]
    for k, name in RES.items():
        v = next((ln.split()[-1] for ln in block if ln.split()[:1] == [".amdhsa_" + name]), None)
        c[k] = int(v) if v is not None and v.lstrip("-").isdigit() else v
    return c


def main():
    args = sys.argv[1:]
    pat = re.compile(args[args.index("--kernels") + 1]) if "--kernels" in args else re.compile(".")
    out = {}
    for a in args:
        if "=" not in a:
            continue
        name, d = a.split("=", 1)
        out[name] = {}
        for f in sorted(glob.glob(os.path.join(d, "*-hip-amdgcn-*gfx950.s"))):
            unit = os.path.basename(f).split("-hip-")[0]
            for k, (body, block) in sorted(kernels(open(f).read()).items()):
                if pat.search(k):
                    out[name][unit + ":" + k] = count(body, block)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
