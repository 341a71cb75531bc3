"""``w4_linear`` -- the weight-only MXFP4 linear layer for few rows ("MXFP4 forward for few rows") -- on the GPU.

Shapes (M, K, F): one row / one k step / narrowest output; M % 16 != 0, F % 64 != 0, three k steps (the prefetch ring wraps with a remainder);
a row block holding one row at FLUX's K; the many-row instantiation with a column tile partly outside F; and for every block height the
launcher picks (16 .. 128 rows) a block filled exactly and one row over.  (a) fp64 segments inside helpers.MLP_SEG_BOUND on bytes covering
all 256 nibble pairs with scale bytes 119 .. 135 (every widened value a normal bf16 number); (b) known integer answers, bit for bit, equal to
``F.linear`` over ``W4Linear.widened()``; (c) the contract on sentinel buffers, pitch, repeat launches, zero bias, row independence;
(d) ``W4Linear.forward`` under ``mlp.w4_stream_rows``."""
import pytest
import torch

from helpers import MLP_SEG_BOUND, assert_segs_close

pytestmark = pytest.mark.gpu

SENT = 7.0
EDGES = [(m + d, 128, f) for m, f in ((16, 8), (32, 16), (48, 24), (64, 8), (96, 16), (384, 24)) for d in (0, 1)]
SHAPES = [(1, 128, 8), (34, 384, 1032), (129, 3072, 128), (257, 1536, 136)] + EDGES
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


def layer(M, K, F, dev, integer=False):
    """(x, W4Linear with a bias) from a seeded generator: random bytes holding all 256 nibble pairs with scale bytes 119 .. 135, or
    (`integer`) scale byte 128 with 129 in block ``i % (K / 32)`` of row ``i``, integer x and bias"""
    from chipmunk_amd.modules import W4Linear
    g = torch.Generator().manual_seed(M * 7 + K + F)
    w = torch.randint(0, 256, (F, K // 2), generator=g, dtype=torch.uint8)
    w.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    if integer:
        s = torch.full((F, K // 32), 128, dtype=torch.uint8)
        s[torch.arange(F), torch.arange(F) % (K // 32)] = 129
        x, b = torch.randint(-4, 5, (M, K), generator=g).bfloat16(), torch.randint(-8, 9, (F,), generator=g).bfloat16()
    else:
        s = torch.randint(119, 136, (F, K // 32), generator=g, dtype=torch.uint8)
        x, b = torch.randn(M, K, generator=g).bfloat16(), (8 * torch.randn(F, generator=g)).bfloat16()
    return x.to(dev), W4Linear.from_mx(w.to(dev), s.to(dev), b.to(dev))


@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_fp64_and_the_contract(dev, shape, has_bias):
    from chipmunk_amd import ops
    M, K, F = shape
    x, q = layer(M, K, F, dev)
    w, s, b = q.weight.data, q.block_scale, (q.bias.data if has_bias else None)
    # (c) the operator on views of sentinel buffers: x inside a NaN-filled [M + 3, K + 64], y inside [M + 2, F + 24]
    xbuf = torch.full((M + 3, K + 64), float("nan"), dtype=torch.bfloat16, device=dev)
    xbuf[:M, :K] = x
    ybuf = torch.full((M + 2, F + 24), SENT, dtype=torch.bfloat16, device=dev)
    torch.ops.chipmunk.w4_linear(xbuf[:M, :K], w, s, b, ybuf[:M, :F])
    got = ybuf[:M, :F].clone()
    assert torch.isfinite(got.float()).all(), "a NaN row of the x buffer was read"
    assert (ybuf[M:] == SENT).all() and (ybuf[:, F:] == SENT).all(), "sentinels behind y"
    # (a)
    exact = x.double() @ q.widened().double().T + (b.double() if has_bias else 0.0)
    worst = assert_segs_close(got.cpu(), exact.cpu(), MLP_SEG_BOUND, f"w4_linear {shape} bias={has_bias}")
    print(f"w4_linear {shape} bias={has_bias}: worst segment {worst:.4f} (bound {MLP_SEG_BOUND:.4f})")
    # (c) the pitch does not enter the bits; a second launch neither; zero bias = no bias; row independence
    plain = ops.w4_linear(x, w, s, b)
    assert plain.shape == (M, F) and torch.equal(bits(plain), bits(got)), "pitched x against contiguous x"
    assert torch.equal(bits(ops.w4_linear(x, w, s, b)), bits(got)), "two launches"
    if not has_bias:
        assert torch.equal(bits(ops.w4_linear(x, w, s, torch.zeros_like(q.bias.data))), bits(got)), "zero bias = no bias"
    for m in sorted({0, 15, 16, 127, 128, M - 1}):
        if m < M:
            assert torch.equal(bits(ops.w4_linear(x[m:m + 1], w, s, b)[0]), bits(got[m])), f"row {m} differs from the one-row launch"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_known_answers(dev, shape):
    from chipmunk_amd import ops
    x, q = layer(*shape, dev, integer=True)
    wide = q.widened()
    got = ops.w4_linear(x, q.weight.data, q.block_scale, None)
    exact = x.double() @ wide.double().T
    assert float(exact.abs().max()) < 2 ** 24 and (wide.float() == wide.float().round()).all()
    assert torch.equal(bits(got), bits(exact.to(torch.bfloat16))), "integer inputs, no bias: the one rounding of the exact value"
    assert torch.equal(bits(got), bits(torch.nn.functional.linear(x, wide))), "F.linear over the widened weight"
    # with the integer bias: two non-zero x per row keep every sum exact in bf16, whichever way F.linear adds its bias
    xs = torch.zeros_like(x)
    xs[:, [3, x.shape[1] - 2]] = x[:, [3, x.shape[1] - 2]].sign()
    got = ops.w4_linear(xs, q.weight.data, q.block_scale, q.bias.data)
    exact = xs.double() @ wide.double().T + q.bias.data.double()
    assert (exact == exact.to(torch.bfloat16).double()).all(), "the case is exact in bf16"
    assert torch.equal(bits(got), bits(exact.to(torch.bfloat16))), "integer inputs and bias"
    assert torch.equal(bits(got), bits(torch.nn.functional.linear(xs, wide, q.bias.data))), "F.linear with the bias over the widened weight"


def test_w4linear_forward_under_the_key(dev, fresh_config, monkeypatch):
    import chipmunk_amd.ops
    K, F = 384, 1032
    x257, q = layer(257, K, F, dev)
    x34 = x257[:34]
    real, calls = chipmunk_amd.ops.w4_linear, []

    def spy(x, *a, **kw):
        calls.append(tuple(x.shape))
        return real(x, *a, **kw)
    monkeypatch.setattr(chipmunk_amd.ops, "w4_linear", spy)
    off34, off257 = q(x34), q(x257)
    assert fresh_config["mlp"]["w4_stream_rows"] == 0 and calls == [], "with the key at 0 nothing streams"
    assert torch.equal(off34, torch.nn.functional.linear(x34, q.widened(), q.bias))
    fresh_config["mlp"]["w4_stream_rows"] = 256
    on34 = q(x34)
    assert calls == [(34, K)] and torch.equal(bits(on34), bits(real(x34, q.weight, q.block_scale, q.bias))), "the operator's bits"
    assert torch.equal(bits(q(x257)), bits(off257)) and calls == [(34, K)], "more rows than the key: the widened path, the key-off bits"
