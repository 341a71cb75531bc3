"""Ragged token counts in the sparse MLP, the parts that need no GPU: the *_ragged entry points of the C ABI are declared, exported and
listed; their argument checks return codes and messages; the fake kernels give the ragged shapes; the Python fallback of
``modules/mlp.py::block_mean`` takes the mean over the rows present in a ragged last block."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ["chipmunk_csp_mlp_mm1_ragged", "chipmunk_csp_mlp_mm1_scatter_ragged", "chipmunk_csp_mlp_mm1_fp8_ragged",
          "chipmunk_csp_mlp_mm2_ragged", "chipmunk_csp_mlp_mm2_and_scatter_add_ragged", "chipmunk_csp_scatter_add_ragged",
          "chipmunk_block_mean_ragged"]
P = ctypes.c_void_p(16)       # a non-null pointer: every call below fails its argument checks before anything is launched
NULL = ctypes.c_void_p(0)


def test_ragged_entry_points_are_declared_exported_and_listed():
    from chipmunk_amd import _native
    text = open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _native.lib()
    for name in RAGGED + ["chipmunk_transpose16_pitched"]:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/chipmunk_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SYMBOLS
    assert lib.chipmunk_abi_version() == 1


def _calls(M, ldc, ptr=P):
    """name -> call of every ragged entry point that takes a cache pitch, with M rows, K = 256, F = 512, N2 = 256"""
    from chipmunk_amd import _native
    lib = _native.lib()
    return {
        "mm1": lambda: lib.chipmunk_csp_mlp_mm1_ragged(ptr, P, P, P, P, P, P, M, 256, 512, ldc, NULL),
        "mm1_scatter": lambda: lib.chipmunk_csp_mlp_mm1_scatter_ragged(ptr, P, P, P, P, P, P, M, 256, 512, ldc, NULL),
        "mm1_fp8": lambda: lib.chipmunk_csp_mlp_mm1_fp8_ragged(ptr, P, P, P, P, P, P, P, P, M, 256, 512, ldc, 0, NULL),
        "mm2_and_scatter_add": lambda: lib.chipmunk_csp_mlp_mm2_and_scatter_add_ragged(ptr, P, P, P, P, P, P, M, 512, 256, ldc, NULL),
        "scatter_add": lambda: lib.chipmunk_csp_scatter_add_ragged(ptr, P, P, P, M, 512, ldc, NULL),
    }


@pytest.mark.parametrize("M,ldc", [(333, 328), (1000, 992), (333, 333), (333, 340), (129, 0)])
def test_bad_pitch_returns_a_code_and_names_the_rule(M, ldc):
    from chipmunk_amd import _native
    for name, call in _calls(M, ldc).items():
        assert call() == 1, name
        msg = _native.last_error()
        assert "ldc" in msg and "multiple of 8" in msg and "at least M" in msg, (name, msg)


def test_null_pointers_return_a_code():
    from chipmunk_amd import _native
    lib = _native.lib()
    for name, call in _calls(333, 336, ptr=NULL).items():
        assert call() == 1 and "null" in _native.last_error(), name
    assert lib.chipmunk_csp_mlp_mm2_ragged(NULL, P, P, P, P, 333, 512, 256, NULL) == 1 and "null" in _native.last_error()
    assert lib.chipmunk_csp_mlp_mm2_ragged(P, P, P, NULL, P, 333, 512, 256, NULL) == 1 and "indices" in _native.last_error()
    assert lib.chipmunk_block_mean_ragged(NULL, P, ctypes.c_int64(1000), 512, 128, NULL) == 1 and "null" in _native.last_error()
    assert lib.chipmunk_block_mean_ragged(P, P, ctypes.c_int64(0), 512, 128, NULL) == 1
    assert lib.chipmunk_transpose16_pitched(P, P, 1, 1003, 512, 1000, NULL) == 1 and "pitch" in _native.last_error()


def test_the_existing_entries_keep_their_checks():
    from chipmunk_amd import _native
    lib = _native.lib()
    assert lib.chipmunk_csp_mlp_mm1(P, P, P, P, P, P, P, 100, 64, 256, NULL) == 1 and "multiple of 128" in _native.last_error()
    assert lib.chipmunk_csp_scatter_add(P, P, P, P, 1000, 512, 6, NULL) == 1 and "multiple of 128" in _native.last_error()
    assert lib.chipmunk_csp_mlp_mm2(P, P, P, P, P, 1000, 512, 256, NULL) == 1 and "multiple of 128" in _native.last_error()
    assert lib.chipmunk_block_mean(P, P, ctypes.c_int64(1000), 512, 128, NULL) == 1 and "multiple of mbm" in _native.last_error()
    # a ragged M is not refused for being ragged: the first failing check of this call is the one on K
    assert lib.chipmunk_csp_mlp_mm1_ragged(P, P, P, P, P, P, P, 100, 100, 256, 104, NULL) == 1 and "K must be" in _native.last_error()


def test_fake_kernels_give_the_ragged_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(1, 1000, 512, dtype=torch.bfloat16)
        assert torch.ops.chipmunk.block_mean(x, 128).shape == (1, 8, 512)
        assert torch.ops.chipmunk.block_mean(x, 192).shape == (1, 6, 512)
        assert torch.ops.chipmunk.block_mean(x, 125).shape == (1, 8, 512)
        act = torch.empty(1, 1003, 512, dtype=torch.bfloat16)
        t = torch.ops.chipmunk.transpose_last2_pitched(act, 1008)
        assert t.shape == (1, 512, 1008) and t.dtype == torch.bfloat16
        assert torch.ops.chipmunk.transpose_last2(act).shape == (1, 512, 1003)


@pytest.mark.parametrize("n,mbm", [(1000, 128), (1000, 192), (129, 128), (100, 128), (1024, 128)])
def test_block_mean_fallback_takes_the_rows_present(n, mbm):
    from chipmunk_amd.modules.mlp import block_mean
    x = torch.randn(2, n, 24, generator=torch.Generator().manual_seed(n))
    got = block_mean(x, mbm)
    blocks = (n + mbm - 1) // mbm
    assert got.shape == (2, blocks, 24)
    for b in range(blocks):
        assert torch.allclose(got[:, b], x[:, b * mbm:(b + 1) * mbm].mean(dim=1), rtol=1e-6, atol=1e-6)
    if n % mbm == 0:      # whole blocks: the reference's expression, bit for bit
        assert torch.equal(got, x.reshape(2, n // mbm, mbm, 24).mean(dim=2))


def test_module_on_cpu_keeps_a_pitched_cache_for_a_ragged_token_count(fresh_config):
    """The full step of SparseDiffMlp (plain torch on the CPU) stores the activation cache whole at a pitch of ceil8(N) with zeroed padding,
    the output cache as [1, N, C] and the block means as [1, ceil(N / mbm), F]."""
    from chipmunk_amd.modules import SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    cfg = fresh_config
    cfg["offloading"]["global_disable_offloading"] = True
    cfg["mlp"].update(dict(top_keys=0.3, random_keys=0.0, full_step_every=4, first_n_dense_layers=0))
    torch.manual_seed(0)
    N, K, F = 203, 16, 64
    fc1, fc2 = torch.nn.Linear(K, F), torch.nn.Linear(F, K)
    act = torch.nn.GELU(approximate="tanh")
    mlp = SparseDiffMlp(0, LayerCounter(1, 1), fc1, act, fc2, 6)
    x = torch.randn(1, N, K)
    with torch.no_grad():
        out = mlp(x)
        a = act(fc1(x))
    stored = mlp.storage.get_sparse_act_T()
    assert stored.shape == (1, F, 208) and stored.is_contiguous()
    assert torch.equal(stored[..., :N], a.transpose(1, 2)) and (stored[..., N:] == 0).all()
    assert mlp.storage.get_out_cache().shape == (1, N, K) and out.shape == (1, N, K)
    assert mlp.storage.get_blockmean_mid_cache().shape == (1, 2, F)
