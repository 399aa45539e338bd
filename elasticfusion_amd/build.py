"""Builds libefusion_hip.so (hand-written HIP, gfx950 only) in-tree with hipcc.

    python -m elasticfusion_amd.build [--force]
    python -m elasticfusion_amd.build --variant <name> [-D...]      (development / A-B builds: VARIANTS below)

ONE library is shipped (csrc/ef_build.hpp):
    libefusion_hip.so        REFERENCE ROUNDING (no fused multiply-add, the reference's summation order) — every result bit for bit the
                             reference's own sources compiled without contraction; what libefusion.so links and bench.py times
Round 4's build (-DEF_FAST_BUILD: fused multiply-adds + the fast summation order; no faster since round 5 and outside the 1e-4 m / 1e-4 rad
bar on 15 of 113 one-frame checkpoints, profiles/r05_parity_factorial.json) is no longer built by build(): it is the development variant
"fast" (`--variant fast` -> libefusion_hip_fast.so), kept for the parity factorial and the `-m "gpu and fastbuild"` tests.

-ffp-contract=off: fused multiply-adds appear only where the kernels spell them out (fmaf), which is what
makes the integer-valued stages (u16/u8/i16 pyramids, correspondences, index maps) bit-exact against the
CPU oracle (DESIGN.md "Numerics").
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libefusion_hip.so")            # reference rounding (the default)
FAST_LIB = os.path.join(HERE, "libefusion_hip_fast.so")   # build_variant("fast"): NOT part of build() since round 6
NOFMA_LIB = LIB                                           # (rounds 1-4 kept the reference rounding in a test-only libefusion_hip_nofma.so: now the default)
VARIANTS = {   # python -m elasticfusion_amd.build --variant <name>: libefusion_hip_<name>.so
    "fast": ["-DEF_FAST_BUILD"],                               # round 4's shipped build: fused multiply-adds + the fast order (DESIGN_fast_build.md)
    "reforder": ["-DEF_FAST_BUILD", "-DEF_REF_ORDER"],         # fused multiply-adds + the reference's order (round 3's product; parity factorial)
    "nofma_fast": ["-DEF_FORCE_FAST_ORDER"],                   # no fused multiply-adds + the fast order (parity factorial)
    "clocks": ["-DEF_STAGE_CLOCKS"],                           # phase clocks of the default build's tracker (tools/small_clocks.py)
    "fast_clocks": ["-DEF_FAST_BUILD", "-DEF_STAGE_CLOCKS"],   # phase clocks of the fast build's persistent tracker (tools/fast_clocks.py)
    "resolve": ["-DEF_KEEP_INDEX_RESOLVE"],                    # A/B: both predictIndices of a fusing frame resolved into the four index maps (rounds 1-8: two more launches) instead of their consumers tapping the z-buffer keys
}
SHIM_LIB = os.path.join(HERE, "libefusion.so")          # class ElasticFusion (include/ElasticFusion.h) over the C ABI
SOURCES = ["ef_track_kernels.hip", "ef_map_kernels.hip", "ef_context.hip", "ef_ferns.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def needs_build() -> bool:
    if not os.path.exists(LIB) or not os.path.exists(SHIM_LIB):
        return True
    t = os.path.getmtime(LIB)
    root = os.path.dirname(HERE)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".inc", ".hpp", ".h"))]
    deps += [os.path.join(root, "include", "ef_hip.h"), os.path.join(root, "include", "ElasticFusion.h"), os.path.join(root, "include", "efusion_klg.hpp"), os.path.join(root, "include", "efusion_jpeg.hpp"),
             os.path.join(root, "tools", "efusion_replay.cpp"), __file__]
    replay = os.path.join(HERE, "efusion_replay")
    return not os.path.exists(replay) or any(os.path.getmtime(d) > min(t, os.path.getmtime(replay)) for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        cmd = [_hipcc(), *FLAGS, *os.environ.get("EF_HIPCC_FLAGS", "").split(), "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out}")
        if verbose and out.strip():
            print(out)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}")
    # libefusion.so: host-only C++ (compiled by hipcc for the shared __host__ __device__ linear-algebra header)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", SHIM_LIB,
           os.path.join(CSRC, "efusion_shim.hip"), "-L" + HERE, "-lefusion_hip", "-lz", "-ldl", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"libefusion.so build failed:\n{r.stdout}")
    # headless replay front-end (plain g++: it only sees include/ElasticFusion.h)
    replay = os.path.join(HERE, "efusion_replay")
    cmd = ["g++", "-O2", "-std=c++17", os.path.join(os.path.dirname(HERE), "tools", "efusion_replay.cpp"), "-o", replay, "-L" + HERE,
           "-lefusion", "-lefusion_hip", "-lz", "-ldl", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link," + HERE]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"efusion_replay build failed:\n{r.stdout}")
    return LIB


def build_variant(name: str, extra_flags: list[str]) -> str:
    """TEST / DEVELOPMENT builds of libefusion_hip under another name (libefusion_hip_<name>.so, selected with EF_HIP_LIB in the Python
    harness; never loaded by the product).  A name of VARIANTS brings its flags; extra_flags are added."""
    extra_flags = VARIANTS.get(name, []) + list(extra_flags)
    target = os.path.join(HERE, f"libefusion_hip_{name}.so")
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, src.replace(".hip", f"_{name}.o"))
        procs.append((src, subprocess.Popen([_hipcc(), *FLAGS, *extra_flags, "-c", os.path.join(CSRC, src), "-o", obj], stdout=subprocess.PIPE,
                                            stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out}")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", target, *objs, "-Wl,-rpath,/opt/rocm/lib"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}")
    return target


if __name__ == "__main__":
    if "--variant" in sys.argv:   # python -m elasticfusion_amd.build --variant valu -DEF_ACCUM_VALU
        i = sys.argv.index("--variant")
        print(build_variant(sys.argv[i + 1], sys.argv[i + 2:]))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
