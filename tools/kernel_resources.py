#!/usr/bin/env python3
"""Compile csrc/drt_hip.hip for gfx950 (device only, to assembly) and print one line per kernel:
VGPRs, SGPRs, scratch, LDS, occupancy (-Rpass-analysis=kernel-resource-usage), plus -- for the
kernels named on the command line -- an instruction-class histogram of their ISA.

  python tools/kernel_resources.py [--keep DIR] [--against DIR] [--root FILE] [substring of a demangled kernel name ...]

--root FILE: compile FILE in place of csrc/drt_hip.hip, with csrc/ on the include path -- a few lines of explicit instantiations, with
DRT_USER_SHAPES or DRT_SAMPLE_LOSS defined and their headers (drt_user_shapes.h, drt_sample_loss.h) beside it, say: the forms of the path kernels that only hiprtc compiles.

--against DIR (the --keep directory of another build, usually the parent commit's): after the report, one line per kernel saying whether
its resource figures and its instruction stream are the `same` as in that build or which `differs`, then a count of each.  The stream is
compared as text, without comments, blank lines, debug directives, the compilation-unit id symbol and the function's number in its local
labels (.LBB<n>_, .Lfunc_begin<n>, .Lfunc_end<n>, .Ltmp<n>).  The exit status is 1 if a kernel appeared, vanished or changed a figure, or
if a figure was not found in either build.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "drt_hip.hip")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout
    return out.strip().split("\n")


def short(d):
    d = re.sub(r"\(.*", "", d)
    d = d.replace("void ", "")
    return d


def classify(op):
    if op.startswith("v_mfma"): return "mfma"
    if op.startswith(("v_rcp", "v_rsq", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")): return "valu_trans"
    if op.startswith("v_pk_"): return "valu_pk"
    if op.startswith(("v_mul_lo", "v_mul_hi", "v_mad_u64", "v_mad_i64")): return "valu_imul"
    if op.startswith(("v_fma_f64", "v_mul_f64", "v_add_f64", "v_div", "v_rcp_f64", "v_trig", "v_cvt_f64", "v_cvt_f32_f64")): return "valu_f64"
    if op.startswith("v_"): return "valu"
    if op.startswith(("s_load", "s_buffer_load")): return "smem"
    if op.startswith("s_waitcnt"): return "waitcnt"
    if op.startswith(("s_cbranch", "s_branch")): return "branch"
    if op.startswith("s_"): return "salu"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")): return "vmem"
    return "other"


FIGURES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy", "sgpr_spill_count", "vgpr_spill_count")


def parse_asm(path):
    """{mangled name: (figures, instruction stream)} of the kernels in an assembly file: the figures from the kernel's `; Kernel info:`
    comment and its metadata record, the stream from its label to its .amdhsa_kernel block."""
    bodies, figures, kernels = {}, collections.defaultdict(dict), []
    body = info = meta = None
    for line in open(path):
        m = re.match(r"(\S+):\s+; @(\S+)$", line)
        if m and m.group(1) == m.group(2):
            body = bodies[m.group(1)] = []
            last = m.group(1)
            continue
        m = re.match(r"\s+\.amdhsa_kernel (\S+)", line)
        if m:
            kernels.append(m.group(1))
            body = None
        if body is not None:
            code = line.split(";")[0].strip()
            if code and not code.startswith((".loc", ".file", ".cfi_")):
                code = re.sub(r"\.L(func_begin|func_end|tmp)\d+", r".L\1", re.sub(r"\.LBB\d+_", ".LBB_", code))
                body.append(re.sub(r"__hip_cuid_\w+", "__hip_cuid", code))
        if line.startswith("; Kernel info:"):
            info = figures[last]
        elif info is not None:
            m = re.match(r"; (\w+):? *[:=] *(\d+)", line)
            if m:
                info[m.group(1)] = m.group(2)
            elif not line.startswith(";"):
                info = None
        if line.startswith("  - ."):              # a kernel's metadata record: its fields in name order
            meta = {}
        m = re.match(r"\s+(?:- )?\.(name|sgpr_spill_count|vgpr_spill_count):\s+(\S+)", line)
        if m and meta is not None:
            meta[m.group(1)] = m.group(2)
            if len(meta) == 3:
                figures[meta.pop("name")].update(meta)
                meta = None
    return {k: (tuple(figures[k].get(f, "?") for f in FIGURES), bodies[k]) for k in kernels}


def compare(asm, parent_asm):
    new, old = parse_asm(asm), parse_asm(parent_asm)
    names = sorted(set(new) | set(old))
    count = collections.Counter()
    print(f"\nagainst {parent_asm}\n{'kernel':110s} {'figures':>8s} {'stream':>8s}")
    for k, dn in zip(names, demangle(names)):
        if k not in old or k not in new:
            verdict = ("appeared", "") if k in new else ("vanished", "")
            count[verdict[0]] += 1
        else:
            verdict = tuple("same" if new[k][i] == old[k][i] else "differs" for i in (0, 1))
            if "?" in new[k][0] + old[k][0]:          # a figure the parser did not find is no agreement
                verdict = ("unknown", verdict[1])
            count["figures " + verdict[0]] += 1
            count["stream " + verdict[1]] += 1
        print(f"{short(dn)[:110]:110s} {verdict[0]:>8s} {verdict[1]:>8s}")
        if verdict[0] == "differs":
            print("    " + ", ".join(f"{f} {o} -> {n}" for f, o, n in zip(FIGURES, old[k][0], new[k][0]) if o != n))
    print(f"\n{len(new)} kernels ({len(old)} there): " + ", ".join(f"{v} {c}" for c, v in sorted(count.items())))
    return 1 if count["appeared"] or count["vanished"] or count["figures differs"] or count["figures unknown"] else 0


def main():
    args = sys.argv[1:]
    opt = {"--keep": None, "--against": None, "--root": None}
    while args and args[0] in opt:
        if len(args) < 2:
            sys.exit(f"{args[0]} needs a {'file' if args[0] == '--root' else 'directory'}")
        opt[args[0]] = args[1]
        args = args[2:]
    keep, against, root = opt["--keep"], opt["--against"], opt["--root"]
    d = keep or tempfile.mkdtemp(prefix="drt_isa_")
    os.makedirs(d, exist_ok=True)
    asm = os.path.join(d, "drt.s")
    subprocess.run([sys.executable, os.path.join(os.path.dirname(SRC), "embed_sources.py")], check=True)   # (drt_jit_sources.inc, which drt_hip.hip includes)
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.dirname(SRC)] + (["-I" + os.path.dirname(os.path.abspath(root))] if root else []) + ["--cuda-device-only", "-S", "-o", asm, root or SRC, "-Rpass-analysis=kernel-resource-usage"] + \
          [a for a in os.environ.get("DRT_EXTRA_FLAGS", "").split() if a]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stderr)
        sys.exit(1)
    kernels = []
    cur = None
    for line in res.stderr.splitlines():
        m = re.search(r"remark: +(\w[\w \[\]/]*): +(\S+)", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k in ("Function Name", "Name"):
            cur = {"name": v}
            kernels.append(cur)
        elif cur is not None:
            cur[k] = v
    names = demangle([k["name"] for k in kernels])
    print(f"{'kernel':78s} {'VGPR':>5s} {'AGPR':>5s} {'SGPR':>5s} {'scratch':>8s} {'LDS':>7s} {'occ':>4s} {'sgpr-spill':>10s}")
    for k, dn in zip(kernels, names):
        k["short"] = short(dn)
        print(f"{k['short'][:78]:78s} {k.get('VGPRs', '?'):>5s} {k.get('AGPRs', '?'):>5s} {k.get('TotalSGPRs', k.get('SGPRs', '?')):>5s} "
              f"{k.get('ScratchSize [bytes/lane]', '?'):>8s} {k.get('LDS Size [bytes/block]', '?'):>7s} {k.get('Occupancy [waves/SIMD]', '?'):>4s} {k.get('SGPRs Spill', '?'):>10s}")
    status = compare(asm, os.path.join(against, "drt.s")) if against else 0
    if not args:
        return status
    text = open(asm).read()
    for k in kernels:
        if not any(a in k["short"] for a in args):
            continue
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*s_endpgm" % re.escape(k["name"]), text, re.S | re.M)
        if not m:
            continue
        hist = collections.Counter()
        for line in m.group(1).splitlines():
            line = line.strip()
            if not line or line.startswith((";", ".", "//")) or line.endswith(":"):
                continue
            hist[classify(line.split()[0])] += 1
        print(f"\n{k['short']}: static instruction mix")
        for c, n in hist.most_common():
            print(f"  {c:12s} {n}")
    print(f"\nassembly kept in {asm}")
    return status


if __name__ == "__main__":
    sys.exit(main())
