"""The three row-wise norm kernels -- ``qkv_split_norm_kernel`` (csrc/indexed_io.hip), ``split_heads_rownorm_kernel`` and
``residual_ln_modulate_kernel`` (csrc/rowwise.hip) -- against the fp64 definitions of tests/rowwise_model.py, evaluated on the device,
on the input families that reach eps, single heads and columns, and the kernels' own edges (docs/TEST_SENSITIVITY.md, "Row-wise norm
kernels").  Every case asserts, through ``helpers.assert_rowwise_close``: a finite output, bit equality of the copied parts, exactly zero
where the exact segment is zero, and the segment bound of its class -- ``MARGIN * floor`` with the floors tests/test_rowwise_metric_cpu.py
pins on the CPU paths, or the worst case of the roundings for a segment of a handful of elements (`rowwise_model.few_element_segments`).
The assertions of tests/test_gpu_reorder.py and tests/test_gpu_wan_glue.py against the CPU paths stay beside these."""
import ctypes

import pytest
import torch

import rowwise_model as rm
from helpers import assert_rowwise_close

pytestmark = pytest.mark.gpu

FAMILIES = ("ladder", "head_ladder", "special")
SENT = -1.5          # bf16 0xbfc0: no kernel output here is a whole buffer of it


@pytest.fixture()
def dev(fresh_config):
    import chipmunk_amd  # noqa: F401
    return torch.device("cuda:0")


def _vp(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


# ------------------------------------------------------------------------------------------------ qkv_split_norm
def _head_case(dev, family, n, heads, extra, weights, rope, seed, sweep=None):
    x = rm.rms_inputs(family, 1, n, heads, 3, extra, seed, wide=False, sweep=sweep, device=dev)[0]
    qw, kw = (rm.rms_weight(128, torch.bfloat16, seed + 1, dev), rm.rms_weight(128, torch.bfloat16, seed + 2, dev)) if weights else (None, None)
    fc, fs = rm.rope_tables(rope, seed + 3, dev)
    return x, qw, kw, fc, fs


def _check_head(got, x, qw, kw, heads, fc, fs, rope, what):
    n = x.shape[0]
    exact = rm.rms_head_exact(x, qw, kw, heads, rm.EPS, fc, fs)
    rot = rm.rotated_tokens(1, heads, n, rope, device=x.device)
    for name, o, e in zip("qkv", got, exact):
        assert o.shape == (1, heads, n, 128) and o.dtype == torch.bfloat16 and o.is_contiguous()
        if name == "v":
            assert_rowwise_close(o, e, 0.0, f"qkv_split_norm {what} v", copy_of=e.to(torch.bfloat16))
        else:
            assert_rowwise_close(o, e, rm.bound_head(rot, e)[0], f"qkv_split_norm {what} {name}")


@pytest.mark.parametrize("weights", [True, False], ids=["weights", "no weights"])
@pytest.mark.parametrize("n,heads,extra", rm.QKV_SHAPES)
def test_qkv_split_norm_segments(dev, n, heads, extra, weights):
    """(1, 1): one segment.  (37, 3, +64): a wider projection row.  (1200, 4): several workgroups.  (3700, 24): 266 400 segments, the capped
    grid's second sweep (262 144 segments per sweep), with the special rows in it."""
    from chipmunk_amd.ops.qkv import qkv_split_norm
    sweep = rm.QKV_SWEEP_TOKENS if heads == 24 else None
    for family in FAMILIES:
        for rope in rm.rope_row_choices(n):
            x, qw, kw, fc, fs = _head_case(dev, family, n, heads, extra, weights, rope, 1000 + n + rope, sweep)
            got = qkv_split_norm(x, qw, kw, heads, rm.EPS, fc, fs)
            torch.cuda.synchronize()
            _check_head(got, x, qw, kw, heads, fc, fs, rope, f"{family} n{n} h{heads} rope {rope}{' w' if weights else ''}")


def test_qkv_split_norm_writes_nothing_outside_its_outputs(dev):
    from chipmunk_amd import _native
    from chipmunk_amd.ops.qkv import qkv_split_norm
    n, heads, rope = 37, 3, 35
    x, qw, kw, fc, fs = _head_case(dev, "special", n, heads, 64, True, rope, 77)
    size, pad = heads * n * 128, 256
    buf = torch.full((3 * size + 4 * pad,), SENT, dtype=torch.bfloat16, device=dev)
    outs = [buf[pad + p * (size + pad): pad + p * (size + pad) + size] for p in range(3)]
    rc = _native.lib().chipmunk_qkv_split_norm(_vp(x), ctypes.c_int64(x.stride(0)), _vp(qw), _vp(kw), _vp(outs[0]), _vp(outs[1]), _vp(outs[2]),
                                               ctypes.c_int64(n), ctypes.c_int(heads), ctypes.c_float(rm.EPS), _vp(fc), _vp(fs), ctypes.c_int64(rope),
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "chipmunk_qkv_split_norm")
    torch.cuda.synchronize()
    keep = torch.ones_like(buf, dtype=torch.bool)
    for p in range(3):
        keep[pad + p * (size + pad): pad + p * (size + pad) + size] = False
    assert (buf[keep] == SENT).all(), "elements outside q, k, v were written"
    got = [o.view(1, heads, n, 128) for o in outs]
    _check_head(got, x, qw, kw, heads, fc, fs, rope, "sentinel")
    for a, b in zip(got, qkv_split_norm(x, qw, kw, heads, rm.EPS, fc, fs)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ------------------------------------------------------------------------------------------------ split_heads_rownorm
def _wide_case(dev, family, B, n, heads, parts, kind, rope, seed, extra=0, sweep=None, pad_rows=0):
    x = rm.rms_inputs(family, B, n + pad_rows, heads, parts, extra, seed, wide=True, sweep=sweep, device=dev)
    norm, flags = rm.wide_flags(parts, rope)
    ws = rm.wide_weights(kind, norm, heads * 128, seed + 1, dev)
    fc, fs = rm.rope_tables(rope, seed + 4, dev)
    return x, ws, norm, flags, fc, fs


def _check_wide(got, x, heads, ws, norm, flags, fc, fs, rope, what):
    B, n = x.shape[0], x.shape[1]
    exact = rm.rms_row_exact(x, heads, ws, norm, flags, rm.EPS, fc, fs)
    assert len(got) == len(norm)
    for p, (o, e) in enumerate(zip(got, exact)):
        assert o.shape == (B, heads, n, 128) and o.dtype == torch.bfloat16 and o.is_contiguous()
        if not norm[p]:
            assert_rowwise_close(o, e, 0.0, f"split_heads_rownorm {what} part {p} copy", copy_of=e.to(torch.bfloat16))
        else:
            kind = rm.weight_kind(ws[p])
            rot = rm.rotated_tokens(B, heads, n, rope, flags[p], device=x.device)
            assert_rowwise_close(o, e, rm.bound_wide(kind, rot, e)[0], f"split_heads_rownorm {what} part {p} {kind}")


def _run_wide(x, heads, ws, norm, flags, fc, fs):
    from chipmunk_amd.ops import split_heads_rownorm
    out = split_heads_rownorm(x, heads, ws, norm, flags, rm.EPS, fc, fs)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", list(rm.WIDE_WEIGHTS))
@pytest.mark.parametrize("heads", rm.WIDE_HEADS)
def test_split_heads_rownorm_segments(dev, heads, kind):
    """heads: NV 1, 2, 3, 4, 9, 10, 11, 16, both sides of the HELD switch of fp32 weights (NV <= 10), a clamped tail vector with one, two and
    three heads missing (heads mod 4 = 3, 2, 1).  Parts 1, 2, 3 with the flags of tests/test_gpu_wan_glue.py; rope_rows over
    {0, 1, n, 299}; 64 heads: a wider row (+64 columns)."""
    n = 300
    ropes = {1: (n, 299, 1), 2: (0, 0, 0), 3: (299, 1, n)}
    for parts in (1, 2, 3):
        for f, family in enumerate(FAMILIES):
            rope = ropes[parts][f]
            x, ws, norm, flags, fc, fs = _wide_case(dev, family, 1, n, heads, parts, kind, rope, 2000 + heads * 10 + parts, extra=64 if heads == 64 else 0)
            got = _run_wide(x, heads, ws, norm, flags, fc, fs)
            _check_wide(got, x, heads, ws, norm, flags, fc, fs, rope, f"{family} h{heads} parts {parts} rope {rope}")


@pytest.mark.parametrize("B,n,heads,parts,sweep", [(1, 2800, 3, 3, 2732), (2100, 5, 5, 1, 8192)])
def test_split_heads_rownorm_second_sweep_and_row_walk(dev, B, n, heads, parts, sweep):
    """(1, 2800, 3 parts): 8 400 items over 2 049 workgroups, a wave's second row is 2 732 further.  (2100, 5, 1 part): 10 500 rows over
    2 048 workgroups, RowWalk steps with b_step = 1 638 and tok_step = 2, and wraps (tok >= n)."""
    for family in FAMILIES:
        rope = n if parts == 1 else next(r for r in range(n - 1, 0, -1) if r % 4)
        x, ws, norm, flags, fc, fs = _wide_case(dev, family, B, n, heads, parts, "mixed", rope, 3000 + B, sweep=sweep)
        got = _run_wide(x, heads, ws, norm, flags, fc, fs)
        _check_wide(got, x, heads, ws, norm, flags, fc, fs, rope, f"{family} B{B} n{n} h{heads} parts {parts} rope {rope}")


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_split_heads_rownorm_batch_strided_view(dev, kind):
    B, n, heads, parts, rope = 2, 300, 12, 3, 297
    x, ws, norm, flags, fc, fs = _wide_case(dev, "ladder", B, n, heads, parts, kind, rope, 3500, pad_rows=100)
    view = x[:, :n]                                                                     # batch stride (n + 100) * cols
    assert not view.is_contiguous()
    got = _run_wide(view, heads, ws, norm, flags, fc, fs)
    _check_wide(got, view, heads, ws, norm, flags, fc, fs, rope, f"ladder strided view {kind}")


def test_split_heads_rownorm_writes_nothing_outside_its_outputs(dev):
    from chipmunk_amd import _native
    B, n, heads, parts, rope = 2, 37, 5, 3, 35
    x, ws, norm, flags, fc, fs = _wide_case(dev, "special", B, n, heads, parts, "mixed", rope, 3600, extra=64)
    size, pad = B * heads * n * 128, 256
    buf = torch.full((3 * size + 4 * pad,), SENT, dtype=torch.bfloat16, device=dev)
    outs = [buf[pad + p * (size + pad): pad + p * (size + pad) + size] for p in range(3)]
    code = {"none": 0, "bf16": 1, "fp32": 2}
    mask = lambda bits: ctypes.c_uint(sum(1 << p for p in range(parts) if bits[p]))      # noqa: E731
    rc = _native.lib().chipmunk_split_heads_rownorm(
        _vp(x), ctypes.c_int64(x.stride(0)), ctypes.c_int64(x.stride(1)), ctypes.c_int(parts),
        _vp(ws[0]), ctypes.c_int(code[rm.weight_kind(ws[0])]), _vp(ws[1]), ctypes.c_int(code[rm.weight_kind(ws[1])]), _vp(ws[2]),
        ctypes.c_int(code[rm.weight_kind(ws[2])]), _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), mask(norm), mask(flags), ctypes.c_int64(B), ctypes.c_int64(n),
        ctypes.c_int(heads), ctypes.c_float(rm.EPS), _vp(fc), _vp(fs), ctypes.c_int64(rope), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "chipmunk_split_heads_rownorm")
    torch.cuda.synchronize()
    keep = torch.ones_like(buf, dtype=torch.bool)
    for p in range(3):
        keep[pad + p * (size + pad): pad + p * (size + pad) + size] = False
    assert (buf[keep] == SENT).all(), "elements outside the three outputs were written"
    got = [o.view(B, heads, n, 128) for o in outs]
    _check_wide(got, x, heads, ws, norm, flags, fc, fs, rope, "sentinel")
    for a, b in zip(got, _run_wide(x, heads, ws, norm, flags, fc, fs)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ------------------------------------------------------------------------------------------------ residual_ln_modulate
def _check_ln(ox, oxm, x, y, gate, shift, scale, what):
    if y is not None:
        bad = rm.nearest_bf16_violations(ox, rm.residual_exact(x, y, gate))
        assert bad == 0, f"{what}: {bad} elements of x_out are no nearest bf16 of the fp64 x + gate * y"
    else:
        assert ox.data_ptr() == x.data_ptr() or torch.equal(ox, x)
    exact, prod = rm.ln_modulate_exact(x, y, gate, shift, scale, x_out=ox if y is not None else None, with_prod=True)
    assert oxm.shape == x.shape and oxm.dtype == torch.bfloat16
    assert_rowwise_close(oxm, exact, rm.bound_ln(exact, prod)[0], f"residual_ln_modulate {what}", width=rm.SEG_W)


def _run_ln(x, y, gate, shift, scale):
    from chipmunk_amd.ops.qkv import residual_ln_modulate
    out = residual_ln_modulate(x, y, gate, shift, scale, rm.EPS)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("rows,cols,residual", [(rm.LN_ROWS, c, r) for c in rm.LN_COLS for r in (True, False)] + [(8209, 1024, True), (8209, 8, False)])
def test_residual_ln_modulate_segments(dev, rows, cols, residual):
    """cols 8 .. 5128: nv 1, 2, 3, 6, 7, 11 on templates 2, 3, 6, 10, 16, the last vector partly or wholly past the row; 3072 and 8192 fit
    exactly.  8 209 rows: the row walk's second step (8 192 waves), a ragged last sweep, special rows in it -- with the residual at 1 024
    columns and without at 8."""
    for family in ("ladder", "special"):
        x, y, gate, shift, scale = rm.ln_inputs(family, rows, cols, residual, 4000 + cols, sweep=8192 if rows > 8192 else None, device=dev)
        ox, oxm = _run_ln(x, y, gate, shift, scale)
        _check_ln(ox, oxm, x, y, gate, shift, scale, f"{family} {rows}x{cols}{' residual' if residual else ''}")


def test_residual_ln_modulate_writes_nothing_outside_its_outputs(dev):
    from chipmunk_amd import _native
    rows, cols = 70, 520
    x, y, gate, shift, scale = rm.ln_inputs("special", rows, cols, True, 4500, device=dev)
    size, pad = rows * cols, 256
    buf = torch.full((2 * size + 3 * pad,), SENT, dtype=torch.bfloat16, device=dev)
    ox, oxm = buf[pad: pad + size], buf[2 * pad + size: 2 * pad + 2 * size]
    rc = _native.lib().chipmunk_residual_ln_modulate(_vp(x), _vp(y), _vp(gate), _vp(shift), _vp(scale), _vp(ox), _vp(oxm), ctypes.c_int64(rows),
                                                     ctypes.c_int(cols), ctypes.c_double(rm.EPS), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "chipmunk_residual_ln_modulate")
    torch.cuda.synchronize()
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[pad: pad + size] = False
    keep[2 * pad + size: 2 * pad + 2 * size] = False
    assert (buf[keep] == SENT).all(), "elements outside x_out and xm were written"
    _check_ln(ox.view(rows, cols), oxm.view(rows, cols), x, y, gate, shift, scale, "sentinel")
    rx, rxm = _run_ln(x, y, gate, shift, scale)
    assert torch.equal(rx.view(torch.int16), ox.view(rows, cols).view(torch.int16)) and torch.equal(rxm.view(torch.int16), oxm.view(rows, cols).view(torch.int16))
