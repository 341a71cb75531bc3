"""Are the single-sequence (B == 1) kernels of csrc/mlp.hip the same machine code in two trees?

    python tools/mlp_isa_diff.py OTHER_MLP_HIP [THIS_MLP_HIP]

compiles both sources with ``hipcc --offload-arch=gfx950 -O3 -S`` (device side only; needs no GPU), cuts every kernel's instruction
stream out of the assembly, normalises what a rename moves (mangled symbol names, local label numbers, comments) and compares the streams of
the kernels both trees have: GEMM1 bf16, GEMM1 fp8, GEMM2 and scatter-add as the existing entry points launch them.  A kernel is matched by
its demangled name with the trailing ``BATCHED = false`` template argument and the parameter list dropped; the GEMM1 kernels of a tree from
before ``mm1_form_kernel`` (``mm1_act_kernel``, ``mm1_rs_kernel``, ``mm1_glu_kernel``, ``mm1_glu_fp8_kernel``) are matched with the
``mm1_form_kernel`` instantiation that took their place.  Also prints the register counts
of every kernel of both trees.  Exit status 0: every shared kernel is instruction-for-instruction identical.
"""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "chipmunk_amd", "csrc")
# the GEMM1 kernels that became mm1_form_kernel: old name -> its (FP8, GLU, RS) arguments (FP8 None: the old kernel's own fifth argument)
FORMS = {"mm1_act_kernel": (None, "false", "false"), "mm1_rs_kernel": ("true", "false", "true"),
         "mm1_glu_kernel": ("false", "true", "false"), "mm1_glu_fp8_kernel": ("true", "true", "false")}


def assembly(src: str) -> str:
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "mlp.s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", f"-I{CSRC}",
                               f"-I{os.path.join(HERE, '..', 'include')}", "-x", "hip", src, "-o", out], stderr=subprocess.DEVNULL, cwd=d)
        return open(out).read()


def key(mangled: str) -> str:
    """mm1_kernel<128, 64, 2, 2, false, 4, false>(...) and mm1_kernel<128, 64, 2, 2, false, 4>(...) -> the same key; the batched
    instantiations (..., true>) keep their own."""
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    m = re.match(r"(\w+)(<[^>]*>)?", name)
    base, targs = m.group(1), m.group(2) or ""
    args = [a.strip() for a in targs[1:-1].split(",")]
    if base in FORMS:    # a tree from before mm1_form_kernel<BN, BK, NST, WPS, FP8, GLU, ACT, RS, BATCHED>: the kernel's name said the form
        fp8, glu, rs = FORMS[base]
        shape, (act, batched) = args[:4], args[-2:]
        base, args = "mm1_form_kernel", shape + [args[4] if fp8 is None else fp8, glu, act, rs, batched]
        targs = "<" + ", ".join(args) + ">"
    if base in ("mm1_kernel", "mm2_kernel"):
        full = 7 if base == "mm1_kernel" else 6
        if len(args) == full and args[-1] == "false":
            args = args[:-1]
        targs = "<" + ", ".join(args) + ">"
    if targs == "<>":      # scatter_add_kernel<>: no batch stride = the kernel the other tree calls scatter_add_kernel
        targs = ""
    return base + targs


def kernels(text: str):
    """key -> (normalised instruction lines, {metadata field: value})"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
        mangled, body = m.group(1), m.group(2)
        lines = []
        for ln in body.split("\n"):
            ln = re.sub(r";.*$", "", ln).strip()
            if not ln or ln.startswith(".") and not ln.startswith(".LBB"):
                continue
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"_Z\w+", "SYM", ln)
            lines.append(ln)
        meta = {}
        mm = re.search(r"\.name:\s+%s\n(.*?)\.wavefront_size" % re.escape(mangled), text, flags=re.S)
        if mm:
            for f in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
                v = re.search(r"\.%s:\s+(\d+)" % f, mm.group(1))
                meta[f] = int(v.group(1)) if v else None
        out[key(mangled)] = (lines, meta)
    return out


def main(argv):
    other = argv[1]
    this = argv[2] if len(argv) > 2 else os.path.join(CSRC, "mlp.hip")
    ko, kt = kernels(assembly(other)), kernels(assembly(this))
    bad = 0
    for k in sorted(set(ko) | set(kt)):
        if k in ko and k in kt:
            same = ko[k][0] == kt[k][0]
            bad += not same
            print(f"{'IDENTICAL' if same else 'DIFFERENT'}  {k}: {len(ko[k][0])} / {len(kt[k][0])} lines; other {ko[k][1]}; this {kt[k][1]}")
            if not same and len(ko[k][0]) == len(kt[k][0]):     # same length: show what moved (e.g. kernel-argument offsets of a grown struct)
                for a, b in [(a, b) for a, b in zip(ko[k][0], kt[k][0]) if a != b][:8]:
                    print(f"           - {a}\n           + {b}")
        else:
            side, v = ("other only", ko[k]) if k in ko else ("this only", kt[k])
            print(f"{side:10} {k}: {len(v[0])} lines; {v[1]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
