"""``residual_ln_modulate_f32_kernel`` (csrc/rowwise.hip), Wan's block glue, against the fp64 definition of
tests/wan_block_glue_model.py evaluated on the device.  Every case asserts: a finite output; ``x_out`` bit-equal to torch's fp32
``x.float() + y.float() * gate``; every 128-column segment of ``xm`` within ``MARGIN`` x the floor of its class (pinned on the CPU path by
tests/test_wan_block_glue_cpu.py; the worst case of the roundings for a segment of a handful of elements), through
``helpers.assert_rowwise_close``; sentinel bytes around both outputs untouched; a batch of two equal to two launches of one sequence
bit for bit; a graph replay equal to the eager call.  docs/TEST_SENSITIVITY.md, "Wan block glue"."""
import ctypes

import pytest
import torch

import wan_block_glue_model as gm
from helpers import assert_rowwise_close

pytestmark = pytest.mark.gpu

FAMILIES = ("ladder", "special")
SENT = -1.5          # bf16 0xbfc0, fp32 0xbfc00000: no kernel output here is a whole buffer of it
PAD = 256


@pytest.fixture()
def dev(fresh_config):
    import chipmunk_amd  # noqa: F401
    return torch.device("cuda:0")


def _vp(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _stride(v, C):
    return C if v is not None and v.dim() > 1 and v.shape[0] > 1 else 0


def _run(t):
    from chipmunk_amd.ops import residual_ln_modulate_f32
    out = residual_ln_modulate_f32(**t, eps=gm.EPS)
    torch.cuda.synchronize()
    return out


def _run_c_abi(t):
    """The C entry writing into sentinel-filled buffers: (x_out or None, xm), after asserting that nothing around them was written."""
    from chipmunk_amd import _native
    x, y = t["x"], t["y"]
    B, L, C = x.shape
    size = x.numel()
    fbuf = torch.full((size + 2 * PAD,), SENT, dtype=torch.float32, device=x.device) if y is not None else None
    hbuf = torch.full((size + 2 * PAD,), SENT, dtype=torch.bfloat16, device=x.device)
    ox = fbuf[PAD: PAD + size] if y is not None else None
    oxm = hbuf[PAD: PAD + size]
    rc = _native.lib().chipmunk_residual_ln_modulate_f32(
        _vp(x), ctypes.c_int(1 if x.dtype == torch.bfloat16 else 2), _vp(y), _vp(t["gate"]), ctypes.c_int64(_stride(t["gate"], C)),
        _vp(t["shift"]), _vp(t["scale"]), ctypes.c_int64(_stride(t["shift"], C)), _vp(t["weight"]), _vp(t["bias"]), _vp(ox), _vp(oxm),
        ctypes.c_int64(B), ctypes.c_int64(L), ctypes.c_int(C), ctypes.c_double(gm.EPS), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "chipmunk_residual_ln_modulate_f32")
    torch.cuda.synchronize()
    for buf, name in ((fbuf, "x_out"), (hbuf, "xm")):
        if buf is not None:
            assert (buf[:PAD] == SENT).all() and (buf[PAD + size:] == SENT).all(), f"elements outside {name} were written"
    return (None if ox is None else ox.view(B, L, C)), oxm.view(B, L, C)


def _check(t, ox, oxm, what):
    x, y, gate = t["x"], t["y"], t["gate"]
    assert oxm.shape == x.shape and oxm.dtype == torch.bfloat16
    if y is not None:
        assert ox.shape == x.shape and ox.dtype == torch.float32
        assert torch.equal(ox.view(torch.int32), gm.residual_f32(x, y, gate).view(torch.int32)), f"{what}: x_out is not torch's fp32 x + y * gate"
    cls = gm.rounding_class(x, y, t["weight"] is not None)
    exact, prod = gm.glue_exact(x, y, gate, t["shift"], t["scale"], t["weight"], t["bias"], x_out=ox if y is not None else None, with_prod=True)
    assert_rowwise_close(oxm, exact, gm.bound(cls, exact, prod)[0], f"residual_ln_modulate_f32 {what}", width=gm.SEG_W)


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                                              b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))


def _sequence(t, b):
    """the inputs of sequence b alone"""
    pick = lambda v: v if v is None or v.dim() == 1 else v[b:b + 1] if v.shape[0] > 1 else v      # noqa: E731
    return dict(x=t["x"][b:b + 1].contiguous(), y=None if t["y"] is None else t["y"][b:b + 1].contiguous(), gate=pick(t["gate"]),
                shift=pick(t["shift"]), scale=pick(t["scale"]), weight=t["weight"], bias=t["bias"])


def _graph_replay(t):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(t)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                            # one stream, one branch
        from chipmunk_amd.ops import residual_ln_modulate_f32
        captured = residual_ln_modulate_f32(**t, eps=gm.EPS)
    for o in captured[1:] if t["y"] is None else captured:
        o.fill_(SENT)
    g.replay()
    torch.cuda.synchronize()
    return captured


@pytest.mark.parametrize("xdtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", gm.COLS)
def test_every_form_at_every_width(dev, C, xdtype):
    """C: NV 1, 2, 3, 3, 6, 10, 11, 16 -- a vector reaches past the row at all but 1536, 5120 and 8192; the vectors are held in registers
    up to 2568 and re-read per row from 5120.  B = 2, L = 35: a wave's row walk crosses the sequence boundary off a multiple of four.
    Forms: no y / gated / ungated residual x modulation [C] / [B, C] (gate [B, 1, C]) / affine."""
    B, L = gm.BATCH, gm.SEQ_LEN
    seed = 9000 + C
    for residual in gm.RESIDUALS:
        if gm.refused(xdtype, residual):
            continue
        for mod in gm.MODS:
            for family in FAMILIES:
                seed += 1
                what = f"{family} C{C} {'bf16' if xdtype == torch.bfloat16 else 'fp32'} {residual} {mod}"
                t = gm.glue_inputs(family, B, L, C, xdtype, residual, mod, seed, device=dev)
                ox, oxm = _run_c_abi(t)
                _check(t, ox, oxm, what)
                wx, wxm = _run(t)                                      # the torch operator: the same bits
                assert _same(wxm, oxm) and (wx is t["x"] if t["y"] is None else _same(wx, ox)), what
            # (on the special family) a batch of two is two launches, and a graph replay is the eager call
            for b in range(B):
                sx, sxm = _run(_sequence(t, b))
                assert _same(sxm[0], wxm[b]) and (t["y"] is None or _same(sx[0], wx[b])), f"{what}: sequence {b} alone"
            gx, gxm = _graph_replay(t)
            assert _same(gxm, wxm) and (t["y"] is None or _same(gx, wx)), f"{what}: graph replay"


def test_second_grid_sweep(dev):
    """8 400 rows of 520 columns over the launcher's 2 048 workgroups: a wave's second row is 8 192 further, in the last sequence of
    three, with the special rows in it."""
    B, L, C = gm.SWEEP_CASE
    for family in FAMILIES:
        t = gm.glue_inputs(family, B, L, C, torch.float32, "gated", "seq", 9900, sweep=8192, device=dev)
        ox, oxm = _run_c_abi(t)
        _check(t, ox, oxm, f"{family} B{B} L{L} C{C} second sweep")


def test_two_wan_blocks_chained(dev):
    """The four uses of a block (model.py:324-334), two blocks in a row, with random bf16 stand-ins for the attention / FFN outputs:
    norm1 + modulate of the bf16 stream; gated residual + affine norm3 (the stream turns fp32); ungated residual + norm2 + modulate; gated
    residual + the next block's norm1 + modulate.  Against the CPU path: the stream bit for bit, xm inside the bound."""
    from chipmunk_amd.ops import residual_ln_modulate_f32 as f
    B, L, C = 2, 35, 1536
    g = torch.Generator().manual_seed(4242)
    x = (torch.randn(B, L, C, generator=g) * 2).to(torch.bfloat16)
    e = [torch.randn(B, 6, C, generator=g) for _ in range(3)]                       # two blocks and what follows them
    w3, b3 = [1 + 0.3 * torch.randn(C, generator=g) for _ in range(2)], [torch.randn(C, generator=g) for _ in range(2)]
    ys = [torch.randn(B, L, C, generator=g).to(torch.bfloat16) for _ in range(6)]
    steps = [dict(y=None, gate=None, shift=e[0][:, 0], scale=e[0][:, 1], weight=None, bias=None)]
    for k in range(2):
        steps += [dict(y=ys[3 * k], gate=e[k][:, 2:3], shift=None, scale=None, weight=w3[k], bias=b3[k]),
                  dict(y=ys[3 * k + 1], gate=None, shift=e[k][:, 3], scale=e[k][:, 4], weight=None, bias=None),
                  dict(y=ys[3 * k + 2], gate=e[k][:, 5:6], shift=e[k + 1][:, 0], scale=e[k + 1][:, 1], weight=None, bias=None)]
    xc, xg = x, x.to(dev)
    for i, s in enumerate(steps):
        sg = {k: (None if v is None else v.contiguous().to(dev)) for k, v in s.items()}
        tg = dict(x=xg, **sg)
        xc, mc = f(xc, **{k: (None if v is None else v.contiguous()) for k, v in s.items()}, eps=gm.EPS)
        xg, mg = f(xg, **sg, eps=gm.EPS)
        torch.cuda.synchronize()
        assert xg.dtype == xc.dtype and _same(xg.cpu(), xc), f"use {i}: the stream differs from the CPU path"
        _check(tg, xg if s["y"] is not None else None, mg, f"chained use {i}")
        assert (mg.cpu().float() - mc.float()).abs().max() <= 2.0 ** -6 * mc.float().abs().max(), f"use {i}: xm far from the CPU path"
    assert xg.dtype == torch.float32
