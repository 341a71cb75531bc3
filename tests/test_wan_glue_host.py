"""Wan's attention operands without a GPU: ``chipmunk.ops.split_heads_rownorm`` (row-wide q / k RMSNorm + three-axis rotary + head-major
layout, reference ``examples/wan/wan/modules/model.py:81-97, 49-78, 154-164``) and ``wan_rope_table``.  The reference's Wan module imports
``diffusers``, which is not a dependency of this project, so nothing here is recorded from it: the formulas are pinned by the file:line
of the lines they restate.  The CPU path of the operator is checked against an independent formulation, the table builder against
``torch.polar``, the fake kernel by a full-graph trace, the C entry point's refusals through ctypes, and the compiled kernel's resources
from its ISA."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chipmunk_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ------------------------------------------------------------------------------------------------ the independent formulation
def _formula(x, heads, parts, weights, norm, rope, eps, angles):
    """Written from model.py's lines on its own, one (batch, part) slice at a time and head-major from the start: fp32 row statistics
    over ALL heads*128 channels, ``.type_as``, the weight product in torch's promoted dtype, then ``view_as_complex(x64) *
    polar(1, angle)`` for the first ``len(angles)`` tokens, fp32, bf16.  ``angles`` is fp64 ``[rows, 64]``; the operator takes the
    multiplier as fp32 tables, so the polar value is rounded to fp32 once before the product (the tables ARE that rounding)."""
    B, n, C = x.shape[0], x.shape[1], heads * 128
    outs = []
    for p in range(parts):
        res = torch.empty(B, heads, n, 128, dtype=torch.bfloat16)
        for b in range(B):
            t = x[b, :, p * C:(p + 1) * C].clone()                                     # [n, C] bf16
            if norm[p]:
                tf = t.to(torch.float32)
                ms = (tf * tf).mean(dim=-1, keepdim=True)
                t = (tf * (1.0 / torch.sqrt(ms + eps))).to(torch.bfloat16)             # rsqrt = 1 / sqrt, IEEE
                if weights[p] is not None:
                    t = t * weights[p]                                                 # bf16 x bf16 -> bf16; bf16 x fp32 -> fp32
            t = t.reshape(n, heads, 128).transpose(0, 1)                               # [heads, n, 128]
            if rope[p] and angles is not None and angles.shape[0] > 0:
                rows = angles.shape[0]
                mult = torch.polar(torch.ones_like(angles), angles).to(torch.complex64).to(torch.complex128)   # [rows, 64]
                z = torch.view_as_complex(t[:, :rows].to(torch.float64).reshape(heads, rows, 64, 2).contiguous()) * mult
                head = torch.view_as_real(z).reshape(heads, rows, 128).to(torch.float32)
                t = torch.cat([head, t[:, rows:].to(torch.float32)], dim=1)
            res[b] = t.to(torch.bfloat16)
        outs.append(res)
    return outs


def _tables(angles):
    """The operator's table format from fp64 angles ``[rows, 64]``: fp32 ``[rows, 128]``, a pair's value in both of its entries."""
    fr = torch.polar(torch.ones_like(angles), angles)
    return fr.real.float().repeat_interleave(2, dim=1).contiguous(), fr.imag.float().repeat_interleave(2, dim=1).contiguous()


def _inputs(B, n, heads, parts, wdtype, seed, extra=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, n, parts * heads * 128 + extra, generator=g) * 1.7).to(torch.bfloat16)
    norm = [p < 2 for p in range(parts)] if parts > 1 else [True]
    weights = [(1 + 0.1 * torch.randn(heads * 128, generator=g)).to(wdtype) if norm[p] and wdtype is not None else None for p in range(parts)]
    return x, weights, norm, g


@pytest.mark.parametrize("B,n,heads,parts", [(1, 300, 12, 3), (2, 64, 40, 3), (1, 50, 3, 1), (1, 33, 5, 2)])
@pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rope_frac", [0, 1, 2])
def test_cpu_path_is_bit_equal_to_the_independent_formula(B, n, heads, parts, wdtype, rope_frac):
    from chipmunk_amd.ops import split_heads_rownorm
    x, weights, norm, g = _inputs(B, n, heads, parts, wdtype, seed=1000 * n + heads)
    rope_rows = (0, n // 2, n)[rope_frac]
    angles = torch.rand(rope_rows, 64, generator=g, dtype=torch.float64) * 6.28 - 3.14
    fc, fs = _tables(angles)
    rope = list(norm)                                                                  # q, k rotated; v (and nothing else) copied
    got = split_heads_rownorm(x, heads, weights, norm, rope, 1e-6, fc, fs)
    ref = _formula(x, heads, parts, weights, norm, rope, 1e-6, angles)
    assert len(got) == parts
    for p in range(parts):
        assert got[p].shape == (B, heads, n, 128) and got[p].dtype == torch.bfloat16 and got[p].is_contiguous()
        assert torch.equal(got[p].view(torch.int16), ref[p].view(torch.int16)), f"part {p}"
    if parts == 3:                                                                     # v: the bits of the input
        C = heads * 128
        assert torch.equal(got[2], x[:, :, 2 * C:3 * C].reshape(B, n, heads, 128).permute(0, 2, 1, 3))
    # a 2-D input is batch 1
    if B == 1:
        got2 = split_heads_rownorm(x[0], heads, weights, norm, rope, 1e-6, fc, fs)
        assert all(torch.equal(a, b) for a, b in zip(got, got2))


def test_row_wide_normalisation_is_not_per_head_normalisation():
    """Head h of the input scaled by 2^(h mod 8 - 4): a per-head norm (``qkv_split_norm``, even with the row weight's per-head slices
    broadcast in) undoes the scale, the row-wide norm keeps it -- the results differ by factors, not by rounding."""
    from chipmunk_amd.ops import qkv_split_norm, split_heads_rownorm
    heads, n = 12, 96
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, n, 3, heads, 128, generator=g)
    x = (x * torch.tensor([2.0 ** (h % 8 - 4) for h in range(heads)]).view(1, 1, 1, heads, 1)).to(torch.bfloat16).reshape(1, n, 3 * heads * 128)
    got = split_heads_rownorm(x, heads, (None, None, None), (True, True, False), (False, False, False), 1e-6)
    ref = _formula(x, heads, 3, [None] * 3, [True, True, False], [False] * 3, 1e-6, None)
    for p in range(3):
        assert torch.equal(got[p].view(torch.int16), ref[p].view(torch.int16))
    per_head = qkv_split_norm(x[0], torch.ones(128, dtype=torch.bfloat16), torch.ones(128, dtype=torch.bfloat16), heads, 1e-6)
    for p in range(2):
        rel = ((got[p].float() - per_head[p].float()).abs() / per_head[p].float().abs().clamp_min(1e-3))
        assert rel.median() > 0.3, "row-wide and per-head normalisation must differ by far more than the 1.6e-2 tolerance of the GPU tests"
        # per head: every head has unit RMS; row-wide: head h keeps its 2^(h mod 8 - 4) against the row's RMS
        rms = got[p].float().pow(2).mean(dim=(0, 2, 3)).sqrt()
        assert torch.allclose(rms[1] / rms[0], torch.tensor(2.0), rtol=0.1) and torch.allclose(rms[7] / rms[0], torch.tensor(128.0), rtol=0.1)
    assert torch.equal(got[2], per_head[2])


def test_argument_errors_of_the_python_wrapper():
    from chipmunk_amd.ops import split_heads_rownorm
    x = torch.zeros(1, 4, 3 * 128, dtype=torch.bfloat16)
    t = torch.zeros(4, 128)
    with pytest.raises(ValueError):
        split_heads_rownorm(x, 1, (None, None, torch.ones(128)), (True, True, False))     # weight on a part that is not normalised
    with pytest.raises(ValueError):
        split_heads_rownorm(x, 1, rope=(True, True, False))                               # rotation without tables
    with pytest.raises(ValueError):
        split_heads_rownorm(x, 1, freqs_cos=t)                                            # one table
    with pytest.raises(ValueError):
        split_heads_rownorm(x, 65)
    with pytest.raises(ValueError):
        split_heads_rownorm(x, 1, norm=(True,) * 4)


# ------------------------------------------------------------------------------------------------ wan_rope_table
def _polar_freqs(length, dim, theta=10000):
    """rope_params (model.py:37-44) for positions 0 .. length-1."""
    ang = torch.outer(torch.arange(length, dtype=torch.float64), 1.0 / torch.pow(theta, torch.arange(0, dim, 2, dtype=torch.float64) / dim))
    return torch.polar(torch.ones_like(ang), ang)


def test_rope_table_columns_follow_frame_height_width():
    from chipmunk_amd.ops import wan_rope_table
    f, h, w = 5, 7, 9
    cos, sin = wan_rope_table((f, h, w), None)
    assert cos.shape == sin.shape == (f * h * w, 128) and cos.dtype == sin.dtype == torch.float32
    for tab in (cos.view(f, h, w, 128), sin.view(f, h, w, 128)):
        assert torch.equal(tab[..., 0::2], tab[..., 1::2])                              # a pair's value in both entries
        assert torch.equal(tab[:, :, :, :44], tab[:, :1, :1, :44].expand(f, h, w, 44))          # first 44 columns: the frame only
        assert torch.equal(tab[:, :, :, 44:86], tab[:1, :, :1, 44:86].expand(f, h, w, 42))      # next 42: the height only
        assert torch.equal(tab[:, :, :, 86:], tab[:1, :1, :, 86:].expand(f, h, w, 42))          # last 42: the width only
        assert not torch.equal(tab[1, 0, 0, :44], tab[0, 0, 0, :44]) and not torch.equal(tab[0, 1, 0, 44:86], tab[0, 0, 0, 44:86])
        assert not torch.equal(tab[0, 0, 1, 86:], tab[0, 0, 0, 86:])
    # the values: rope_params with the 44 / 42 / 42 split of model.py:501-503, rounded once
    ff, fh, fw = _polar_freqs(f, 44), _polar_freqs(h, 42), _polar_freqs(w, 42)
    assert ff.shape[1] == 22 and fh.shape[1] == 21
    assert torch.equal(cos.view(f, h, w, 128)[:, 0, 0, 0:44:2], ff.real.float()) and torch.equal(sin.view(f, h, w, 128)[0, :, 0, 44:86:2], fh.imag.float())
    assert torch.equal(sin.view(f, h, w, 128)[0, 0, :, 86::2], fw.imag.float())
    assert wan_rope_table((f, h, w), None)[0] is cos                                    # cached per arguments


def test_applying_the_table_is_the_polar_product():
    """split_heads_rownorm with wan_rope_table's tables == x64 (complex) * polar(1, angle) of rope_apply (model.py:61-73), the
    multiplier rounded to the tables' fp32 once, then fp32, then bf16: bit-equal."""
    from chipmunk_amd.ops import split_heads_rownorm, wan_rope_table
    f, h, w, heads = 3, 4, 5, 2
    n = f * h * w
    cos, sin = wan_rope_table((f, h, w), None)
    ff, fh, fw = _polar_freqs(f, 44), _polar_freqs(h, 42), _polar_freqs(w, 42)
    freqs = torch.cat([ff.view(f, 1, 1, -1).expand(f, h, w, -1), fh.view(1, h, 1, -1).expand(f, h, w, -1),
                       fw.view(1, 1, w, -1).expand(f, h, w, -1)], dim=-1).reshape(n, 1, 64)         # model.py:63-68
    freqs = freqs.to(torch.complex64).to(torch.complex128)
    x = (torch.randn(1, n, heads * 128, generator=torch.Generator().manual_seed(3)) * 1.3).to(torch.bfloat16)
    got = split_heads_rownorm(x, heads, (None,), (False,), (True,), 1e-6, cos, sin)[0]
    z = torch.view_as_complex(x[0].to(torch.float64).reshape(n, heads, 64, 2)) * freqs
    ref = torch.view_as_real(z).flatten(2).float().to(torch.bfloat16).permute(1, 0, 2).unsqueeze(0)
    assert torch.equal(got.view(torch.int16), ref.contiguous().view(torch.int16))


def test_voxel_ordered_table_is_the_voxel_chunk_of_the_raster_one():
    from chipmunk_amd.ops import wan_rope_table
    from chipmunk_amd.ops.voxel import voxel_chunk_no_padding
    f, h, w = 9, 13, 17                                                                 # tails on all three axes of (4, 6, 8)
    raster = wan_rope_table((f, h, w), None)
    vox = wan_rope_table((f, h, w))                                                     # default voxel shape (4, 6, 8), model.py:70
    for r, v in zip(raster, vox):
        want = voxel_chunk_no_padding(r.view(1, 1, f, h, w, 128), voxel_shape=(4, 6, 8))[0, 0]
        assert v.shape == (f * h * w, 128) and torch.equal(v, want)
    assert not torch.equal(vox[0], raster[0])


# ------------------------------------------------------------------------------------------------ fake kernel
def test_fake_kernel_shapes_and_full_graph_trace():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 100, 3 * 12 * 128 + 64, dtype=torch.bfloat16)
        w = torch.empty(12 * 128, dtype=torch.float32)
        t = torch.empty(80, 128, dtype=torch.float32)
        q, k, v = torch.ops.chipmunk.split_heads_rownorm(x, 12, 3, w, w, None, 3, 3, 1e-6, t, t)
        assert q.shape == k.shape == v.shape == (2, 12, 100, 128) and q.dtype == torch.bfloat16 and q.is_contiguous()
        (k2,) = torch.ops.chipmunk.split_heads_rownorm(x[0], 12, 1, None, None, None, 1, 0, 1e-6)
        assert k2.shape == (1, 12, 100, 128)

    def step(x, w, t):
        q, k, v = torch.ops.chipmunk.split_heads_rownorm(x, 12, 3, w, w, None, 3, 3, 1e-6, t, t)
        return q.float() + k.float(), v

    with FakeTensorMode(allow_non_fake_inputs=True):                                    # (no kernel runs: fake inputs all the way)
        x = torch.empty(2, 100, 3 * 12 * 128, dtype=torch.bfloat16)
        w = torch.empty(12 * 128, dtype=torch.float32)
        t = torch.empty(80, 128, dtype=torch.float32)
        a, b = torch.compile(step, backend="eager", fullgraph=True)(x, w, t)
        assert a.shape == b.shape == (2, 12, 100, 128) and a.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ C ABI
def _call(lib, *, x=4096, bs=0, rs=3 * 12 * 128, parts=3, w=(0, 0, 0), wd=(0, 0, 0), out=(4096, 8192, 12288), norm=3, rope=0, B=1, n=16, heads=12,
          fc=0, fs=0, rope_rows=0):
    p = ctypes.c_void_p
    return lib.chipmunk_split_heads_rownorm(p(x), ctypes.c_int64(bs), ctypes.c_int64(rs), ctypes.c_int(parts), p(w[0]), ctypes.c_int(wd[0]),
                                            p(w[1]), ctypes.c_int(wd[1]), p(w[2]), ctypes.c_int(wd[2]), p(out[0]), p(out[1]), p(out[2]),
                                            ctypes.c_uint(norm), ctypes.c_uint(rope), ctypes.c_int64(B), ctypes.c_int64(n), ctypes.c_int(heads),
                                            ctypes.c_float(1e-6), p(fc), p(fs), ctypes.c_int64(rope_rows), p(0))


def test_c_entry_point_is_exported_and_refuses_bad_arguments_before_touching_a_gpu():
    """Every refusal returns CHIPMUNK_ERR_INVALID (1) with a message that names the rule; the pointers are made-up addresses, so a
    check that ran after a launch would not return at all.  (This machine has no GPU: no HIP call can have succeeded either.)"""
    from chipmunk_amd import _native
    lib = _native.lib()
    assert hasattr(lib, "chipmunk_split_heads_rownorm") and "chipmunk_split_heads_rownorm" in _native.SYMBOLS
    assert lib.chipmunk_abi_version() == 1
    cases = [
        (dict(heads=0), "heads must be in 1 .. 64"),
        (dict(heads=65, rs=3 * 65 * 128), "heads must be in 1 .. 64"),
        (dict(parts=4), "parts must be 1, 2 or 3"),
        (dict(x=4096 + 2), "16-byte aligned"),
        (dict(out=(4096, 8192 + 8, 12288)), "16-byte aligned"),
        (dict(rs=3 * 12 * 128 + 4), "multiples of 8"),
        (dict(rope=3, fc=4096, rope_rows=4), "come together"),
        (dict(rope=3, fs=4096, rope_rows=4), "come together"),
        (dict(rope=3, fc=4096, fs=8192, rope_rows=17), "rope_rows"),
        (dict(rope=1), "needs freqs_cos"),
        (dict(rs=3 * 12 * 128 - 8), "row stride"),
        (dict(norm=8), "past parts"),
        (dict(w=(0, 0, 4096), wd=(0, 0, 1)), "not normalised"),
        (dict(w=(4096, 0, 0), wd=(3, 0, 0)), "dtype code"),
        (dict(B=0), "B must be"),
    ]
    for kw, msg in cases:
        assert _call(lib, **kw) == 1, kw
        assert msg in _native.last_error(), (kw, _native.last_error())
    assert _call(lib, n=0) == 0                                                          # nothing to do is not an error


# ------------------------------------------------------------------------------------------------ ISA audit
def test_every_instantiation_compiles_without_spills_scratch_or_lds_and_with_16_byte_accesses(tmp_path):
    """In the manner of tests/test_kernel_audit.py: compile rowwise.hip to gfx950 assembly (no GPU needed) and read each
    split_heads_rownorm_kernel instantiation's metadata and body.  One instantiation per ceil(heads / 4) = 1 .. 16."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "rowwise.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(CSRC, "rowwise.hip"),
                           "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    docs = [d for d in re.split(r"\n  - (?=\.)", text[text.index("amdhsa.kernels:"):]) if ".name:" in d]   # one entry per kernel
    seen = set()
    for d in docs:
        name = re.search(r"\.name:\s+(\S+)", d).group(1)
        if "split_heads_rownorm_kernel" not in name:
            continue
        field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", d).group(1))   # noqa: E731
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0 and field("agpr_count") == 0, name
        assert field("private_segment_fixed_size") == 0, f"{name}: scratch"
        assert field("group_segment_fixed_size") == 0, f"{name}: LDS"
        assert not re.search(r"\.uses_dynamic_stack:\s+true", d), name
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, name
        assert not re.search(r"\b(scratch_|ds_read|ds_write|ds_load|ds_store|buffer_store|v_accvgpr)", body), name   # (nor registers parked in the accumulator file)
        narrow = re.findall(r"\bglobal_(?:load|store)_(?:dword|dwordx2|dwordx3|short|ushort|ubyte|byte|sbyte|sshort)\b", body)
        assert not narrow, f"{name}: global accesses narrower than 16 bytes: {sorted(set(narrow))}"
        seen.add(int(re.search(r"kernelILi(\d+)E", name).group(1)))
    assert seen == set(range(1, 17)), seen
