"""Static ISA breakdown of one trace_kernel instance (tuning tool, not product).

Compiles render.hip for gfx950 to assembly with line tables (-g changes no
code: the instruction count is checked against the plain build), then counts
the instructions of one kernel by class (VALU, SALU, vector memory, LDS,
scalar memory, branches, waits) and by the source region of their innermost
location: the functions of render.hip and of the headers it includes, keyed
on (file, line), and the sections of trace_body (trace_body.h) between its
RT_STAMP lines.  Static counts weigh
every instruction once; tools/stamps.py gives the dynamic (cycle) shares.

  python tools/isa_breakdown.py [--kernel 1,1,0,0,0,0] [--defs "-DX"] [--asm file.s]
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-swift-raytracer_amd", "csrc")
SRC = os.path.join(CSRC, "render.hip")
TRACE_BODY = os.path.join(CSRC, "trace_body.h")
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "--offload-arch=gfx950",
         "--cuda-device-only", "-S"]


def compile_asm(defs, debug):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = ["/opt/rocm/bin/hipcc"] + FLAGS + (["-g"] if debug else []) + defs + [SRC, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


def kernel_body(lines, flags):
    """Instruction lines (with their .loc) of trace_kernel<flags>."""
    tag = "trace_kernelI" + "".join(("Li%sE" if k == 3 else "Lb%sE") % f for k, f in enumerate(flags)) + "EEvNS_11TraceParamsE:"
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and tag in l)
    body = []
    loc = None
    for l in lines[start + 1:]:
        s = l.strip()
        if s.startswith(".Lfunc_end"):
            break
        if s.startswith(".loc"):
            parts = s.split()
            loc = (int(parts[1]), int(parts[2]))
            continue
        if not s or s.startswith((".", ";")) or s.endswith(":"):
            continue
        body.append((s.split()[0], loc))
    return body


def klass(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "VMEM"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "SMEM"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm")):
        return "branch"
    if op.startswith("s_waitcnt") or op in ("s_nop", "s_barrier", "s_sleep"):
        return "wait/sync"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def unit_files():
    """render.hip and the headers of csrc/ it includes, directly or not."""
    seen, todo = [], [SRC]
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(f):
            continue
        seen.append(f)
        for inc in re.findall(r'^#include "([^"]+)"', open(f).read(), re.M):
            todo.append(os.path.join(CSRC, inc))
    return seen


def regions():
    """{file name: [(first line, last line, function name)]} of the unit's functions."""
    head = re.compile(r"^(?:\s*(?:static\s+)?(?:__device__|__global__|__host__)|(?:static\s+)?"
                      r"(?:void|hipError_t|uint32_t|size_t|int))\b")
    skip = {"__launch_bounds__", "amdgpu_waves_per_eu", "__attribute__", "if", "for", "while", "trace_threads",
            "trace_waves_per_eu"}
    out = {}
    for f in unit_files():
        src = open(f).read().split("\n")
        starts = []
        for i, l in enumerate(src, 1):
            if not head.match(l) or l.rstrip().endswith(";"):
                continue
            names = [n for n in re.findall(r"(\w+)\s*\(", l) if n not in skip]
            if names:
                starts.append((i, names[0]))
        out[os.path.basename(f)] = [(i, starts[k + 1][0] - 1 if k + 1 < len(starts) else len(src), name)
                                    for k, (i, name) in enumerate(starts)]
    # trace_body is still one function: its sections are what lies between its
    # RT_STAMP(k) lines (the segments tools/stamps.py times), which are code
    name = {1: "ray setup", 2: "walks", 3: "shading", 4: "sample store", 5: "fused resolve", 6: "refill",
            0: "direction normalisation"}
    body = os.path.basename(TRACE_BODY)
    src = open(TRACE_BODY).read().split("\n")
    a, b = next((a, b) for a, b, n in out[body] if n == "trace_body")
    stamps = [(i, int(m.group(1))) for i in range(a, b + 1)
              for m in [re.match(r"\s*RT_STAMP\((\d)\);", src[i - 1])] if m]
    loop = next(i for i in range(a, b + 1) if src[i - 1].strip() == "for (;;) {")
    secs = [(a, loop - 1, "trace_body: entry (LDS staging)")]
    prev = loop
    for i, k in stamps:
        secs.append((prev, i, "trace_body loop: " + name[k]))
        prev = i + 1
    secs.append((prev, b, "trace_body: after the loop"))
    out[body] = [r for r in out[body] if r[2] != "trace_body"] + secs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="1,1,0,0,0,0",
                    help="trace_kernel<kBvh,kLds,kStep,kMesh,kCount,kSerial> flags (default: C2's lean kernel)")
    ap.add_argument("--defs", default="")
    ap.add_argument("--asm", default=None)
    args = ap.parse_args()
    flags = args.kernel.split(",")
    defs = args.defs.split() if args.defs else []
    asm = args.asm or compile_asm(defs, True)
    plain = compile_asm(defs, False)
    body = kernel_body(open(asm).read().split("\n"), flags)
    nplain = len(kernel_body(open(plain).read().split("\n"), flags))
    files = {}
    for l in open(asm):
        if l.lstrip().startswith(".file"):
            p = l.split()
            files[int(p[1])] = p[-3].strip('"') if p[-2] == "md5" else p[-1].strip('"')
    funcs = regions()
    by_class = collections.Counter(klass(op) for op, _ in body)
    by_region = collections.defaultdict(collections.Counter)
    for op, loc in body:
        name = "?"
        if loc is not None:
            base = os.path.basename(files.get(loc[0], "?"))
            name = next((f"{n} ({base})" for a, b, n in funcs.get(base, ()) if a <= loc[1] <= b), base)
            if loc[1] == 0:
                name = "(no line)"
        by_region[name][klass(op)] += 1
    print(f"trace_kernel<{args.kernel}>: {len(body)} instructions with -g, {nplain} without "
          f"({'same code' if len(body) == nplain else 'DIFFERENT code: counts approximate'})")
    print("by class: " + ", ".join(f"{k} {v}" for k, v in by_class.most_common()))
    print(f"{'region (innermost source location)':44s} {'total':>6s} {'VALU':>6s} {'SALU':>6s} "
          f"{'VMEM':>5s} {'LDS':>5s} {'SMEM':>5s} {'br':>5s}")
    for name, c in sorted(by_region.items(), key=lambda kv: -sum(kv[1].values())):
        print(f"{name[:44]:44s} {sum(c.values()):6d} {c['VALU']:6d} {c['SALU']:6d} {c['VMEM']:5d} "
              f"{c['LDS']:5d} {c['SMEM']:5d} {c['branch']:5d}")
    if args.asm is None:
        os.unlink(asm)
    os.unlink(plain)


if __name__ == "__main__":
    sys.exit(main())
