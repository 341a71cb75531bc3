"""Per-sequence key lengths (``k_lens``) without a GPU: the added operators' schemas and fake kernels, the reference's
schemas untouched, the new C-ABI symbols, and the argument errors of the Python layer."""
import pytest
import torch

from test_abi import REFERENCE_SCHEMAS, _declared_symbols

VARLEN_SYMBOLS = ["chipmunk_dense_attn_varlen", "chipmunk_dense_colsum_attn_varlen", "chipmunk_dense_colsum_topk_mask_varlen",
                  "chipmunk_dense_colsum_topk_mask_p_varlen", "chipmunk_topk_mask_varlen", "chipmunk_topk_mask_p_varlen"]
VARLEN_OPS = ["dense_attn_varlen", "dense_colsum_attn_varlen", "dense_colsum_topk_mask_varlen", "dense_colsum_topk_mask_p_varlen",
              "topk_mask_varlen", "topk_mask_p_varlen"]


def test_new_c_abi_symbols_are_declared_and_exported():
    from chipmunk_amd import _native
    lib = _native.lib()
    declared = _declared_symbols()
    for name in VARLEN_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/chipmunk_hip.h"
        assert name in _native.SYMBOLS and hasattr(lib, name), f"{name} is not exported"


def test_reference_schemas_are_unchanged_and_k_lens_lives_in_new_operators():
    import chipmunk_amd  # noqa: F401
    for name, schema in REFERENCE_SCHEMAS.items():
        assert str(getattr(torch.ops.chipmunk, name).default._schema) == schema
    for name in VARLEN_OPS:
        schema = str(getattr(torch.ops.chipmunk, name).default._schema)
        assert "Tensor k_lens" in schema, schema
    # one style: no operator without the suffix grew the argument
    for name in ("dense_attn", "dense_attn_layout", "dense_colsum_attn", "dense_colsum_attn_layout", "topk_mask", "topk_mask_p",
                 "dense_colsum_topk_mask", "dense_colsum_topk_mask_p"):
        assert "k_lens" not in str(getattr(torch.ops.chipmunk, name).default._schema)


def test_fake_kernels_give_shapes_and_dtypes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    ops = torch.ops.chipmunk
    with FakeTensorMode():
        B, H, N, Nk = 2, 3, 400, 448
        q = torch.empty(B, H, N, 128, dtype=torch.bfloat16)
        k = torch.empty(B, H, Nk, 128, dtype=torch.bfloat16)
        kl = torch.empty(B, dtype=torch.int32)
        G = 3
        for tm in (False, True):
            o, l = ops.dense_attn_varlen(q, k, k, kl, tm)
            assert o.shape == q.shape and o.dtype == torch.bfloat16 and l.shape == (B, H, N, 1) and l.dtype == torch.float32
            assert o.stride(-1) == 1 and (o.stride(1) == 128) == tm          # token-major: the [B, H, N, D] view of [B, N, H, D]
            o, cs, l2 = ops.dense_colsum_attn_varlen(q, k, k, l, kl, tm)
            assert o.shape == q.shape and cs.shape == (B, H, G, Nk) and cs.dtype == torch.bfloat16 and l2.shape == l.shape
            o, m, l2 = ops.dense_colsum_topk_mask_varlen(q, k, k, l, kl, 64, 0.01, None, None, tm)
            assert o.shape == q.shape and m.shape == (B, H, G, Nk) and m.dtype == torch.bool and l2.dtype == torch.float32
            o, m, l2 = ops.dense_colsum_topk_mask_p_varlen(q, k, k, l, kl, 64, 0.9, 8, 0.01, None, None, tm)
            assert o.shape == q.shape and m.shape == (B, H, G, Nk) and m.dtype == torch.bool and l2.shape == (B, H, N, 1)
        cs = torch.empty(B, H, G, Nk, dtype=torch.bfloat16)
        assert ops.topk_mask_varlen(cs, kl, 64, 0.0, None, None).shape == cs.shape
        m = ops.topk_mask_p_varlen(cs, kl, 64, 0.9, 8, 0.0, None, None)
        assert m.shape == cs.shape and m.dtype == torch.bool


class _OnGpu:
    """A stand-in for the GPU operand the lengths are checked against: only its device and batch size are looked at."""
    is_cuda, device, shape = True, torch.device("cuda", 0), torch.Size((3, 2, 416, 128))


def test_argument_errors_of_k_lens():
    from chipmunk_amd.ops.attn import check_k_lens
    q = _OnGpu()
    assert check_k_lens(None, q, "t") is None
    with pytest.raises(ValueError, match="int32"):
        check_k_lens(torch.zeros(3, dtype=torch.int64), q, "t")          # wrong dtype
    with pytest.raises(ValueError, match="int32"):
        check_k_lens([416, 33, 1], q, "t")                               # not a tensor: lengths never travel through the host
    for bad in (torch.zeros(2, dtype=torch.int32), torch.zeros(3, 1, dtype=torch.int32), torch.zeros(6, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match=r"\[B\]"):
            check_k_lens(bad, q, "t")                                    # wrong length / rank / stride
    with pytest.raises(ValueError, match="device"):
        check_k_lens(torch.zeros(3, dtype=torch.int32), q, "t")          # a CPU k_lens beside GPU operands


def test_cpu_operands_with_k_lens_raise_value_error():
    """The oracle-backed CPU operators are test infrastructure and take no lengths: every public entry refuses them."""
    from chipmunk_amd import ops
    from chipmunk_amd.modules.attn import SparseDiffAttn
    q = torch.zeros(2, 1, 192, 128, dtype=torch.bfloat16)
    kl = torch.tensor([192, 100], dtype=torch.int32)
    l = torch.ones(2, 1, 192, 1)
    cs = torch.zeros(2, 1, 1, 192, dtype=torch.bfloat16)
    calls = [lambda: ops.dense_attn(q, q, q, False, kl), lambda: ops.dense_colsum_attn(q, q, q, l, False, kl),
             lambda: ops.dense_colsum_topk_mask(q, q, q, l, 64, 0.0, None, None, False, kl),
             lambda: ops.dense_colsum_topk_mask_p(q, q, q, l, 64, 0.9, 8, 0.0, None, None, False, kl),
             lambda: ops.topk_mask(cs, 64, 0.0, None, None, kl), lambda: ops.topk_mask_p(cs, 64, 0.9, 8, 0.0, None, None, kl)]
    for call in calls:
        with pytest.raises(ValueError, match="GPU"):
            call()
    layer = SparseDiffAttn.__new__(SparseDiffAttn)      # forward checks the argument before it touches any state
    with pytest.raises(ValueError, match="GPU"):
        SparseDiffAttn.forward(layer, q, q, q, kl)
