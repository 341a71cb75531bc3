"""Compile audit of ``mm1_form_kernel`` (chipmunk_amd/csrc/mlp.hip), the one wrapper kernel of every GEMM1 form but the benchmarked
``mm1_kernel``: one device-only compile of mlp.hip for gfx950, then, from the code object's metadata,

* the instantiations are exactly the thirty the library launches, all at the shipped ``<128, 64, 2, 2>`` shape -- the ungated forms with
  an activation code (bf16 / e4m3, twelve), the e4m3 form with scale vectors (six), the gated bf16 and gated e4m3 forms (six each), each
  over three activations x {single sequence, batch};
* none spills a VGPR, none uses scratch, none declares static LDS (the ring is dynamic LDS, two 32 KiB stages, two workgroups per CU)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MLP_HIP = os.path.join(ROOT, "chipmunk_amd", "csrc", "mlp.hip")

# (FP8, GLU, RS) of the forms; each exists for ACT in 0 .. 2 and BATCHED in 0, 1
FORMS = {"ungated bf16": (0, 0, 0), "ungated fp8": (1, 0, 0), "ungated fp8, scale vectors": (1, 0, 1), "gated bf16": (0, 1, 0),
         "gated fp8": (1, 1, 0)}
EXPECTED = {(f, g, a, r, b) for f, g, r in FORMS.values() for a in (0, 1, 2) for b in (0, 1)}


def test_the_thirty_mm1_form_kernels_compile_without_spills_scratch_or_static_lds(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    assert len(EXPECTED) == 30
    out = tmp_path / "mlp.s"        # (as tests/test_mlp_fp8_fc2_host.py)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", MLP_HIP, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    # mm1_form_kernel<128, 64, 2, 2, FP8, GLU, ACT, RS, BATCHED>: the shipped tile shape only
    shipped = re.compile(r"15mm1_form_kernelILi128ELi64ELi2ELi2ELb([01])ELb([01])ELi([012])ELb([01])ELb([01])EEE")
    seen = set()
    for block in text.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "mm1_form_kernel" not in name.group(1):
            continue
        m = shipped.search(name.group(1))
        assert m, f"an mm1_form_kernel instantiation other than the shipped tile shape: {name.group(1)}"
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spill == 0 and scratch == 0, f"{name.group(1)}: {spill} VGPR spills, {scratch} bytes of scratch"
        assert lds == 0, f"{name.group(1)}: the ring is dynamic LDS"
        form = tuple(int(v) for v in m.groups())
        assert form not in seen, form
        seen.add(form)
    assert seen == EXPECTED, (f"mm1_form_kernel instantiations (fp8, glu, act, rs, batched): missing {sorted(EXPECTED - seen)}, "
                              f"unexpected {sorted(seen - EXPECTED)}")
    # no kernel of the old per-form families is left beside it
    assert not re.search(r"mm1_(act|rs|glu|glu_fp8)_kernel", text)
    # LDS: the kernels declare none statically; the launcher asks for NST * STAGE = 2 * (128 * 128 + 128 * 128) bytes at the one shape
    # every form is launched with
    src = open(MLP_HIP).read()
    assert len(re.findall(r"launch_mm1_variant<128, 64, 2, 2, FP8, 4, BATCHED, GLU, [012], RS>", src)) == 3
    bm, bn, bk, nst = 128, 128, 64, 2
    assert nst * (bm * bk * 2 + bn * bk * 2) <= 64 * 1024, "two workgroups must fit the 160 KiB of a CU"
