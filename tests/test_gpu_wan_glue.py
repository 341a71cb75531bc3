"""``chipmunk.ops.split_heads_rownorm`` on the GPU (``split_heads_rownorm_kernel``, csrc/rowwise.hip) against its CPU path, which is the
reference's own op sequence for Wan's attention operands (``examples/wan/wan/modules/model.py:81-97, 49-78, 154-164``; checked against an
independent formulation in tests/test_wan_glue_host.py).

Unnormalised, unrotated parts (v) are bit copies.  Normalised parts: the kernel adds the row's squares in another order than torch
and rotates in fp32 where the reference rotates in fp64, so a value can land one bf16 step away and the weight product or the
rotation can round that into a second one -- the tolerance of the sibling ``test_qkv_split_norm_matches_the_reference_sequence``
(tests/test_gpu_reorder.py): rtol 1.6e-2, atol 2e-2 with a rotation (a rotated value is a sum of two products: a step of the larger
one can exceed 1.6 % of a small sum) and 1e-6 without, and more than 99 % of the elements equal.  That it holds for the longer sums
here (up to 8192 squares per row instead of 128) was established without a GPU (docs/EXPERIMENTS_r09.md, section 2): an fp32 sum in the
kernel's order and an fp32 rotation, emulated on the CPU against the reference order, left every element inside it and at least
99.99 % equal for 3, 12, 40 and 64 heads and both weight dtypes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

#          B, n,     heads, parts, extra columns, rope_rows
SHAPES = [(1, 32760, 12, 3, 0, 32760),      # Wan 1.3B self-attention
          (2, 4000, 12, 3, 0, 3900),
          (1, 2000, 40, 3, 0, 2000),        # Wan 14B width
          (1, 300, 64, 3, 64, 300),
          (1, 777, 3, 3, 0, 0),             # heads not a multiple of 4
          (1, 512, 12, 2, 0, 0),            # k normalised, v copied: the cross-attention keys (model.py:196-197)
          (1, 1000, 12, 1, 1536, 0),        # one part of a wider row: the cross-attention query (model.py:195)
          (1, 1, 1, 1, 0, 1)]


@pytest.fixture()
def dev(fresh_config):
    import chipmunk_amd  # noqa: F401
    return torch.device("cuda:0")


def _case(B, n, heads, parts, extra, rope_rows, weights, seed=None):
    """x, per-part weights, norm and rope flags, tables: q (and k) normalised -- and rotated when there is a table -- the last part of
    a two- or three-part row copied."""
    g = torch.Generator().manual_seed(n * 131 + heads if seed is None else seed)
    C = heads * 128
    x = (torch.randn(B, n, parts * C + extra, generator=g) * 1.7).to(torch.bfloat16)
    norm = [True] if parts == 1 else [p < parts - 1 for p in range(parts)]
    rope = [nm and rope_rows > 0 for nm in norm]
    kinds = {"none": [None] * 3, "bf16": [torch.bfloat16] * 3, "fp32": [torch.float32] * 3, "mixed": [torch.float32, torch.bfloat16, None]}[weights]
    ws = [(1 + 0.1 * torch.randn(C, generator=g)).to(kinds[p]) if norm[p] and kinds[p] is not None else None for p in range(parts)]
    fc = fs = None
    if rope_rows:
        ang = torch.rand(rope_rows, 64, generator=g, dtype=torch.float64) * 6.28
        fc, fs = ang.cos().float().repeat_interleave(2, dim=1).contiguous(), ang.sin().float().repeat_interleave(2, dim=1).contiguous()
    return x, ws, norm, rope, fc, fs


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _run(dev, x, heads, ws, norm, rope, fc, fs):
    from chipmunk_amd.ops import split_heads_rownorm
    out = split_heads_rownorm(x, heads, _to(dev, *ws), norm, rope, 1e-6, *_to(dev, fc, fs))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("weights", ["bf16", "fp32", "none", "mixed"])
@pytest.mark.parametrize("B,n,heads,parts,extra,rope_rows", SHAPES)
def test_kernel_matches_the_reference_sequence(dev, B, n, heads, parts, extra, rope_rows, weights):
    from chipmunk_amd.ops import split_heads_rownorm
    x, ws, norm, rope, fc, fs = _case(B, n, heads, parts, extra, rope_rows, weights)
    ref = split_heads_rownorm(x, heads, ws, norm, rope, 1e-6, fc, fs)                   # CPU: the reference's op sequence
    got = _run(dev, x.to(dev), heads, ws, norm, rope, fc, fs)
    assert len(got) == parts
    for p in range(parts):
        o = got[p].cpu()
        assert o.shape == (B, heads, n, 128) and o.dtype == torch.bfloat16 and got[p].is_contiguous()
        if not norm[p]:
            assert torch.equal(o.view(torch.int16), ref[p].view(torch.int16)), f"part {p}: a copied part must be bit-exact"
            continue
        same = (o == ref[p]).float().mean().item()
        err = (o.float() - ref[p].float()).abs()
        print(f"part {p}: equal {same:.6f}, max abs err {err.max().item():.3e}, "
              f"max err / (atol + rtol |ref|) {(err / ((2e-2 if rope[p] else 1e-6) + 1.6e-2 * ref[p].float().abs())).max().item():.3f}")
        torch.testing.assert_close(o.float(), ref[p].float(), rtol=1.6e-2, atol=2e-2 if rope[p] else 1e-6)
        assert same > 0.99


def test_a_batch_of_two_is_two_batches_of_one_and_launches_repeat(dev):
    B, n, heads, parts, extra, rope_rows = 2, 4000, 12, 3, 0, 3900
    x, ws, norm, rope, fc, fs = _case(B, n, heads, parts, extra, rope_rows, "fp32")
    xd = x.to(dev)
    both = _run(dev, xd, heads, ws, norm, rope, fc, fs)
    again = _run(dev, xd, heads, ws, norm, rope, fc, fs)
    for p in range(parts):
        assert torch.equal(both[p].view(torch.int16), again[p].view(torch.int16)), "two identical launches must be bit-identical"
    for b in range(B):
        one = _run(dev, xd[b:b + 1].contiguous(), heads, ws, norm, rope, fc, fs)
        flat = _run(dev, xd[b], heads, ws, norm, rope, fc, fs)                           # [n, cols]: batch 1
        for p in range(parts):
            assert torch.equal(both[p][b:b + 1].view(torch.int16), one[p].view(torch.int16)), f"batch {b} part {p}"
            assert torch.equal(one[p].view(torch.int16), flat[p].view(torch.int16))


@pytest.mark.parametrize("weights", ["bf16", "fp32"])
def test_rows_behind_the_table_are_the_rows_of_a_launch_without_tables(dev, weights):
    B, n, heads, parts, extra, rope_rows = 2, 1500, 12, 3, 0, 1000
    x, ws, norm, rope, fc, fs = _case(B, n, heads, parts, extra, rope_rows, weights)
    xd = x.to(dev)
    rot = _run(dev, xd, heads, ws, norm, rope, fc, fs)
    plain = _run(dev, xd, heads, ws, norm, [False] * parts, None, None)
    for p in range(parts):
        assert torch.equal(rot[p][:, :, rope_rows:].view(torch.int16), plain[p][:, :, rope_rows:].view(torch.int16))
        if rope[p]:
            assert not torch.equal(rot[p][:, :, :rope_rows], plain[p][:, :, :rope_rows])


def test_columns_behind_the_parts_are_never_read(dev):
    B, n, heads, parts, extra, rope_rows = 2, 300, 5, 3, 64, 300
    x, ws, norm, rope, fc, fs = _case(B, n, heads, parts, extra, rope_rows, "bf16")
    C = heads * 128
    clean = _run(dev, x.to(dev), heads, ws, norm, rope, fc, fs)
    x[:, :, parts * C:] = float("nan")
    dirty = _run(dev, x.to(dev), heads, ws, norm, rope, fc, fs)
    for p in range(parts):
        assert not torch.isnan(dirty[p].float()).any()
        assert torch.equal(clean[p].view(torch.int16), dirty[p].view(torch.int16))


def test_a_batch_strided_view_gives_the_bits_of_its_contiguous_copy(dev):
    B, n, heads, parts, extra, rope_rows = 2, 700, 12, 3, 0, 650
    x, ws, norm, rope, fc, fs = _case(B, n + 100, heads, parts, extra, rope_rows, "fp32")
    xd = x.to(dev)
    view = xd[:, :n]                                                                    # batch stride (n + 100) * cols
    assert not view.is_contiguous()
    a = _run(dev, view, heads, ws, norm, rope, fc, fs)
    b = _run(dev, view.contiguous(), heads, ws, norm, rope, fc, fs)
    for p in range(parts):
        assert a[p].shape == (B, heads, n, 128)
        assert torch.equal(a[p].view(torch.int16), b[p].view(torch.int16))


def test_rotation_without_normalisation_and_empty_input(dev):
    """The three settings of a part are independent (qk_norm=False in model.py:135-136 leaves a rotation alone), and n = 0 is legal."""
    from chipmunk_amd.ops import split_heads_rownorm
    x, ws, norm, rope, fc, fs = _case(1, 200, 12, 1, 0, 150, "none")
    ref = split_heads_rownorm(x, 12, (None,), (False,), (True,), 1e-6, fc, fs)
    got = _run(dev, x.to(dev), 12, [None], (False,), (True,), fc, fs)
    torch.testing.assert_close(got[0].cpu().float(), ref[0].float(), rtol=1.6e-2, atol=2e-2)
    assert (got[0].cpu() == ref[0]).float().mean() > 0.99
    assert torch.equal(got[0].cpu()[:, :, 150:], x[:, 150:].reshape(1, 50, 12, 128).permute(0, 2, 1, 3))
    empty = _run(dev, x[:, :0].to(dev), 12, [None], (True,), (False,), None, None)
    assert empty[0].shape == (1, 12, 0, 128)
