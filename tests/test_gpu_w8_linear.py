"""``w8_linear`` -- the weight-only fp8 linear layer for few rows ("Weight-only forward for few rows") -- on the GPU.

Shapes (M, K, F): (1, 64, 8) one row, one k step, the narrowest output; (34, 192, 1032) an F that is no multiple of the 64-column tile and
an M that is no multiple of 16; (129, 3072, 1024) a second row block holding one row, FLUX's K; (257, 1536, 2048) three row blocks, Wan's K;
(128, 64, 16) a row block that is exactly full; and, for the block heights the launcher picks, (96, 64, 16) / (97, 128, 24) a 96-row block
full and one row over, (385, 128, 136) a fourth 128-row block of one row under two column tiles per wave.  At each, with one scale and a
vector of scales, with and without a bias:
(a) every 64-column segment of every row within helpers.MLP_SEG_BOUND of the fp64 model (tests/w8_linear_model.py) on inputs that hold
    every finite e4m3 byte -- the bound the CPU definition meets with room (FLOOR_W8_LINEAR); no new constant;
(b) known answers: integer inputs whose sums are exact in fp32 give the one rounding of the exact value, bit for bit, and the bits of
    ``F.linear`` over the widened weight; with an integer bias (and sums small enough for the inner rounding to be exact) as well;
(c) a zero bias gives the bits of no bias, a constant vector of scales those of the number; row m of the M-row launch has the bits of the
    one-row launch on ``x[m : m + 1]``; NaN rows of the x buffer at and past M are not read, sentinel rows of y past M and sentinel columns
    between F and ldy are not written; a pitched x (ldx > K) gives the bits of the contiguous one; two launches give the same bits;
(d) ``W8Linear.forward`` under ``mlp.w8_stream_rows``: few rows take the kernel, more rows the widened path with the key-off bits."""
import pytest
import torch

import w8_linear_model as model
from helpers import MLP_SEG_BOUND, assert_segs_close

pytestmark = pytest.mark.gpu

SENT = 7.0
IDS = ["x".join(map(str, s)) for s in model.SHAPES_GPU]


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


def launch(x, w, s, b, pad_k=64, pad_f=24):
    """the operator on views of sentinel buffers: x [M, K] inside a NaN-filled [M + 3, K + pad_k], y [M, F] inside [M + 2, F + pad_f];
    -> (y view, y buffer)"""
    M, K = x.shape
    F = w.shape[0]
    xbuf = torch.full((M + 3, K + pad_k), float("nan"), dtype=torch.bfloat16, device=x.device)
    xbuf[:M, :K] = x
    ybuf = torch.full((M + 2, F + pad_f), SENT, dtype=torch.bfloat16, device=x.device)
    torch.ops.chipmunk.w8_linear(xbuf[:M, :K], w, s, b, ybuf[:M, :F])
    return ybuf[:M, :F], ybuf


@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("vec", [False, True], ids=["scalar", "vector"])
@pytest.mark.parametrize("shape", model.SHAPES_GPU, ids=IDS)
def test_against_the_fp64_model_and_the_contract(dev, shape, vec, has_bias):
    from chipmunk_amd import ops
    M, K, F = shape
    c = model.case(*shape)
    x, w = c["x"].to(dev), c["w"].to(dev)
    s = (c["sv"] if vec else c["s1"]).to(dev)
    b = c["bias"].to(dev) if has_bias else None
    y, ybuf = launch(x, w, s, b)
    got = y.clone()
    # (c) nothing outside [0, M) x [0, F) is written, nothing at or past M is read
    assert torch.isfinite(got.float()).all(), "a NaN row of the x buffer was read"
    assert (ybuf[M:] == SENT).all() and (ybuf[:, F:] == SENT).all(), "sentinels behind y"
    # (a)
    worst = assert_segs_close(got.cpu(), c["exact"][(vec, has_bias)], MLP_SEG_BOUND, f"w8_linear {shape} vec={vec} bias={has_bias}",
                              width=model.SEG_WIDTH)
    print(f"w8_linear {shape} vec={vec} bias={has_bias}: worst segment {worst:.4f} (bound {MLP_SEG_BOUND:.4f})")
    # (c) the wrapper on the contiguous x: the pitch does not enter the bits; a second launch neither
    plain = ops.w8_linear(x, w, s, b)
    assert plain.shape == (M, F) and torch.equal(bits(plain), bits(got)), "pitched x against contiguous x"
    assert torch.equal(bits(ops.w8_linear(x, w, s, b)), bits(got)), "two launches"
    if has_bias:
        assert torch.equal(bits(ops.w8_linear(x, w, s, torch.zeros_like(b))), bits(ops.w8_linear(x, w, s, None))), "zero bias = no bias"
    if not vec:
        assert torch.equal(bits(ops.w8_linear(x, w, s.expand(F).contiguous(), b)), bits(got)), "a constant vector of scales = the number"
    # (c) row independence
    for m in sorted({0, 15, 16, 127, 128, M - 1}):
        if m < M:
            one = ops.w8_linear(x[m:m + 1], w, s, b)
            assert torch.equal(bits(one[0]), bits(got[m])), f"row {m} of the {M}-row launch differs from the one-row launch"


@pytest.mark.parametrize("shape", model.SHAPES_GPU, ids=IDS)
def test_known_answers(dev, shape):
    from chipmunk_amd import ops
    M, K, F = shape
    c = model.integer_case(*shape)
    w = c["w"].to(dev)
    for e in (-3, 2):                                   # a power-of-two scale, one number and a vector
        s1 = torch.tensor([2.0 ** e], device=dev)
        for s in (s1, s1.expand(F).contiguous()):
            x = c["x"].to(dev)
            got = ops.w8_linear(x, w, s, None)
            exact = model.exact(c["x"], c["w"], s.cpu(), None)
            assert torch.equal(bits(got.cpu()), bits(exact.to(torch.bfloat16))), "integer inputs, no bias: the one rounding of the exact value"
            wide = (c["w"].to(torch.bfloat16) * (2.0 ** e)).to(dev)
            assert torch.equal(bits(got), bits(torch.nn.functional.linear(x, wide))), "F.linear over the widened weight"
    # with an integer bias: sums small enough for both roundings to be exact
    s = torch.tensor([0.5], device=dev)
    xs, b = c["x_sparse"].to(dev), c["bias"].to(dev)
    got = ops.w8_linear(xs, w, s, b)
    exact = model.exact(c["x_sparse"], c["w"], s.cpu(), c["bias"])
    assert (exact == exact.to(torch.bfloat16).double()).all(), "the case is exact in bf16"
    assert torch.equal(bits(got.cpu()), bits(exact.to(torch.bfloat16))), "integer inputs and bias"
    wide = (c["w"].to(torch.bfloat16) * 0.5).to(dev)
    assert torch.equal(bits(got), bits(torch.nn.functional.linear(xs, wide, b))), "F.linear with the bias over the widened weight"


# ------------------------------------------------------------------------------------------------------------------ W8Linear.forward
def _layer(dev, K, F, scaling):
    from chipmunk_amd.modules import W8Linear
    torch.manual_seed(5)
    return W8Linear.from_linear(torch.nn.Linear(K, F).bfloat16().to(dev), scaling=scaling)


@pytest.mark.parametrize("scaling", ["tensor", "row"])
def test_w8linear_forward_under_the_key(dev, fresh_config, monkeypatch, scaling):
    import chipmunk_amd.ops
    K, F = 192, 1032
    q = _layer(dev, K, F, scaling)
    real, calls = chipmunk_amd.ops.w8_linear, []

    def spy(x, *a, **kw):
        calls.append(tuple(x.shape))
        return real(x, *a, **kw)
    monkeypatch.setattr(chipmunk_amd.ops, "w8_linear", spy)
    g = torch.Generator().manual_seed(9)
    x34, x257 = torch.randn(34, K, generator=g).bfloat16().to(dev), torch.randn(257, K, generator=g).bfloat16().to(dev)
    off34, off257 = q(x34), q(x257)
    assert calls == [] and torch.equal(off34, torch.nn.functional.linear(x34, q.widened(), q.bias))
    fresh_config["mlp"]["w8_stream_rows"] = 256
    on34 = q(x34)
    assert calls == [(34, K)] and on34.shape == (34, F) and on34.dtype == torch.bfloat16
    # the layer's value: the fp64 model over (weight, scale_reciprocal, bias), the operator's bound
    exact = model.exact(x34.cpu(), q.weight.data.cpu(), q.scale_reciprocal.cpu(), q.bias.data.cpu())
    assert_segs_close(on34.cpu(), exact, MLP_SEG_BOUND, f"W8Linear.forward 34 rows {scaling}", width=model.SEG_WIDTH)
    assert torch.equal(bits(on34), bits(real(x34, q.weight, q.scale_reciprocal, q.bias)))
    # more rows than the key: the widened path, the key-off bits
    on257 = q(x257)
    assert calls == [(34, K)] and torch.equal(bits(on257), bits(off257))
    # [2, 17, K] is 34 rows
    on3d = q(x34.view(2, 17, K))
    assert calls == [(34, K), (2, 17, K)] and on3d.shape == (2, 17, F) and torch.equal(bits(on3d.view(34, F)), bits(on34))
    # a strided last dimension stays on the widened path
    wide_x = torch.randn(34, 2 * K, generator=g).bfloat16().to(dev)[:, ::2]
    assert wide_x.stride(-1) == 2 and torch.equal(q(wide_x), torch.nn.functional.linear(wide_x, q.widened(), q.bias))
    assert len(calls) == 2
    # a row count at the key still takes the kernel
    fresh_config["mlp"]["w8_stream_rows"] = 257
    q(x257)
    assert calls[-1] == (257, K) and len(calls) == 3
