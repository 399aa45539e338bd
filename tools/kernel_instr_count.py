#!/usr/bin/env python
"""Static instruction counts of the kernels of one HIP source (gfx950, the project's flags; no GPU needed):

    python tools/kernel_instr_count.py <file.hip> [name filter] [extra hipcc flags ...]

Per kernel: instructions in all, VALU (v_*), IEEE float divisions (v_div_fixup), v_div_scale, v_sqrt, v_rcp, DPP moves, vector-memory loads
(global_load*), `s_waitcnt vmcnt` and the code size the assembler reports.  Counted over the `--cuda-device-only -S` text between a kernel's
label and its .Lfunc_end."""
import re
import subprocess
import sys
import tempfile
import os

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]


def main():
    src = sys.argv[1]
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "dev.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, *sys.argv[3:], "--cuda-device-only", "-S", src, "-o", asm])
        text = open(asm).read()
    labels = re.findall(r"^(_Z\w+):\s*;\s*@", text, flags=re.M)
    names = subprocess.run(["c++filt"], input="\n".join(labels), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    for label, name in zip(labels, names):
        name = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "").replace("void ", ""))
        if flt and not re.search(flt, name):
            continue
        body = text[text.index(label + ":"):]
        body = body[:body.index(".Lfunc_end")]
        ins = [ln.split()[0] for ln in body.splitlines()[1:] if ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;")]
        n = lambda pat: sum(1 for i in ins if re.match(pat, i))   # noqa: E731
        dpp = sum(1 for ln in body.splitlines() if re.search(r"\b(quad_perm|row_sh[lr]|row_ror|row_bcast|row_mirror)", ln))
        vm = sum(1 for ln in body.splitlines() if re.search(r"s_waitcnt.*vmcnt", ln))
        size = re.search(r"; codeLenInByte = (\d+)", text[text.index(label + ":"):])
        print(f"{name[:48]:48s} instr={len(ins):5d} valu={n(r'v_'):5d} div={n(r'v_div_fixup'):3d} div_scale={n(r'v_div_scale'):3d} "
              f"sqrt={n(r'v_sqrt'):3d} rcp={n(r'v_rcp'):3d} dpp={dpp:2d} vmem_load={n(r'global_load'):3d} waitcnt_vm={vm:3d} "
              f"code_bytes={size.group(1) if size else '?'}")


if __name__ == "__main__":
    main()
