"""Ragged token counts through the full-size launches and through the SparseDiffMlp module.

Full size, one launch each (GEMM1 with its scatter-add, then GEMM2), the last group and three sampled groups against fp32 torch:
HunyuanVideo 720x1280x129 (M = 119 056 = 930 groups + 16 rows, bf16) and Wan2.1 480x832x81 (M = 32 760 = 255 groups + 120 rows, fp8).
Module: a full step, then a sparse step, at N = 1000 (ldc == N) and N = 1003 (pitched cache)."""
import pytest
import torch

from helpers import assert_close_bf16

pytestmark = pytest.mark.gpu

BM = 128


@pytest.fixture(scope="module")
def dev():
    import chipmunk_amd  # noqa: F401
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name,M,K,F,N2,fp8", [("hunyuan", 119056, 3072, 12288, 3072, False), ("wan", 32760, 1536, 8960, 1536, True)])
def test_full_size_ragged_gemm1_scatter_then_gemm2(dev, name, M, K, F, N2, fp8):
    G = (M + BM - 1) // BM
    assert M % BM != 0 and M % 8 == 0
    # the 32-bit-offset conditions of the entry points hold at both sizes
    assert M * K < 2 ** 31 and F * K < 2 ** 31 and F * M < 2 ** 31 and M * F < 2 ** 31 and F * N2 < 2 ** 31
    g_ = torch.Generator(device=dev).manual_seed(M)
    x = torch.randn(M, K, device=dev, generator=g_) * 0.5
    w = torch.randn(F, K, device=dev, generator=g_) * 0.05
    if fp8:
        sa, sb = 448.0 / x.abs().max(), 448.0 / w.abs().max()
        a, w1 = (x * sa).to(torch.float8_e4m3fn), (w * sb).to(torch.float8_e4m3fn)
        ra, rb = (1.0 / sa).reshape(1).float(), (1.0 / sb).reshape(1).float()
    else:
        a, w1 = x.to(torch.bfloat16), w.to(torch.bfloat16)
    del x, w
    bias = (torch.randn(F, device=dev, generator=g_) * 0.2).to(torch.bfloat16)
    w2T = (torch.randn(F, N2, device=dev, generator=g_) * 0.03).to(torch.bfloat16)
    out0 = (torch.randn(M, N2, device=dev, generator=g_) * 0.5).to(torch.bfloat16)
    cache_buf = torch.empty(F + 1, M, dtype=torch.bfloat16, device=dev)       # ldc == M (M % 8 == 0), one canary row behind
    cache_buf.normal_(generator=g_).mul_(0.3)
    cache_buf[F] = 7.0
    cache = cache_buf[:F]
    sample = sorted({G - 1, 0, G // 3, (2 * G) // 3 + 1})
    cache_before = {g: cache[:, g * BM:min(M, (g + 1) * BM)].clone() for g in sample}
    inds = torch.rand(G, F, device=dev, generator=g_).argsort(dim=1).to(torch.int32)
    counts = (torch.randint(10, 16, (G,), device=dev, generator=g_) * 256).to(torch.int32)      # 2560 .. 3840: about 0.3 F at HunyuanVideo size
    counts[G // 3] = 0
    c_buf = torch.full((M + BM, F), 7.0, dtype=torch.bfloat16, device=dev)
    out_buf = torch.full((M + BM, N2), 7.0, dtype=torch.bfloat16, device=dev)
    c, out = c_buf[:M], out_buf[:M]
    out.copy_(out0)
    if fp8:
        torch.ops.chipmunk.csp_mlp_mm1_fp8_scatter(a, w1, c, bias, cache, inds, counts, ra, rb)
    else:
        torch.ops.chipmunk.csp_mlp_mm1_scatter(a, w1, c, bias, cache, inds, counts)
    torch.ops.chipmunk.csp_mlp_mm2(c, w2T, inds, counts, out)
    torch.cuda.synchronize()
    assert (c_buf[M:] == 7.0).all() and (out_buf[M:] == 7.0).all() and (cache_buf[F] == 7.0).all(), "a canary row changed"
    for g in sample:
        rows = slice(g * BM, min(M, (g + 1) * BM))
        n = int(counts[g])
        assert (c[rows, n:] == 7.0).all(), f"{name} group {g}: packed columns past the count written"
        cols, rest = inds[g, :n].long(), inds[g, n:].long()
        old = cache_before[g]
        assert torch.equal(cache[:, rows][rest], old[rest]), f"{name} group {g}: unselected cache columns changed"
        if n == 0:
            assert torch.equal(out[rows], out0[rows])
            continue
        if fp8:
            acc = (a[rows].float() @ w1[cols].float().T) * ra * rb + bias[cols].float()
            act = torch.nn.functional.gelu(acc, approximate="tanh").to(torch.bfloat16).float()
            want = (act - old[cols].float().T).to(torch.bfloat16)
            tol = dict(atol=3e-2, rtol=3e-2)
        else:
            act = torch.nn.functional.gelu(a[rows].float() @ w1[cols].float().T + bias[cols].float(), approximate="tanh")
            want = act - old[cols].float().T
            tol = {}
        assert_close_bf16(c[rows, :n], want, what=f"{name} GEMM1 group {g} ({rows.stop - rows.start} rows) vs fp32 torch", **tol)
        new = (old[cols].float() + c[rows, :n].float().T).to(torch.bfloat16)
        assert torch.equal(cache[:, rows][cols], new), f"{name} group {g}: cache != bf16(cache + delta)"
        prod = (c[rows, :n].float() @ w2T[cols].float()).to(torch.bfloat16)
        assert_close_bf16(out[rows], prod.float() + out0[rows].float(), what=f"{name} GEMM2 group {g} vs fp32 torch")


def _module(dev, cfg, N, top_keys, fp8, offload):
    from chipmunk_amd.modules import SparseDiffMlp, F8Linear
    from chipmunk_amd.util.layer_counter import LayerCounter
    cfg["offloading"]["global_disable_offloading"] = not offload
    if offload:
        cfg["offloading"]["mlp.sparse_act_T"] = True
        cfg["offloading"]["keep_resident_if_fits"] = False
    cfg["mlp"].update(dict(top_keys=top_keys, random_keys=0.0, full_step_every=4, block_mask_cache=2, first_n_dense_layers=0,
                           counts_multiple_of=256))
    torch.manual_seed(N)
    K, F = 256, 1024
    fc1 = torch.nn.Linear(K, F, device=dev, dtype=torch.bfloat16)
    if fp8:
        fc1 = F8Linear.from_linear(fc1, input_float8_dtype=torch.float8_e4m3fn)
    fc2 = torch.nn.Linear(F, K, device=dev, dtype=torch.bfloat16)
    act = torch.nn.GELU(approximate="tanh")
    mlp = SparseDiffMlp(0, LayerCounter(1, 1), fc1, act, fc2, 6)
    x0 = torch.randn(1, N, K, device=dev, dtype=torch.bfloat16)
    x1 = x0 + 0.3 * torch.randn_like(x0)
    if fp8:
        try:                               # torch._scaled_mm support varies with the ROCm build (as in tests/test_gpu_mlp.py's fp8 module test)
            with torch.no_grad():
                fc1(x0)
        except (RuntimeError, NotImplementedError) as e:
            pytest.skip(f"torch._scaled_mm fp8 unavailable here: {e}")
    return mlp, fc1, fc2, act, x0, x1


def _two_steps(mlp, x0, x1, offload):
    """Full step on x0, sparse step on x1; returns (out0, cache before the sparse step [F, N], out1, cache after it, whole stored cache)."""
    N = x0.shape[1]
    with torch.no_grad():
        out0 = mlp(x0).clone()
        if offload:
            mlp.storage.load_async()
            mlp.storage.load_async_wait()
        stored = mlp.storage.get_sparse_act_T()
        ld = (N + 7) // 8 * 8
        assert stored.shape == (1, mlp.fc1[0].out_features, ld) and stored.is_contiguous(), "the pitched cache is stored (and reloaded) whole"
        assert (stored[..., N:] == 0).all(), "zeroed padding"
        before = stored[0, :, :N].clone()
        out1 = mlp(x1).clone()
        torch.cuda.synchronize()
        after = mlp.storage.get_sparse_act_T()[0, :, :N].clone()
    assert out0.shape == out1.shape == x0.shape[:2] + (mlp.fc2[0].out_features,)
    assert mlp.storage.get_out_cache().shape == out1.shape
    assert mlp.storage.get_blockmean_mid_cache().shape == (1, (N + 127) // 128, mlp.fc1[0].out_features)
    return out0, before, out1, after


@pytest.mark.parametrize("N,fp8,offload", [(1000, False, False), (1003, False, False), (1000, True, False), (1003, False, True)])
def test_module_all_columns_reproduces_the_dense_mlp(dev, fresh_config, N, fp8, offload):
    """top_keys = 1.0: cache + delta == fresh activations, output == dense MLP on the new input (tolerances of
    tests/test_gpu_mlp.py::test_run_e2e_matches_dense_delta)."""
    mlp, fc1, fc2, act, x0, x1 = _module(dev, fresh_config, N, 1.0, fp8, offload)
    out0, before, out1, after = _two_steps(mlp, x0, x1, offload)
    with torch.no_grad():
        act1 = act(fc1(x1))[0]
        ref = fc2(act1)
    assert_close_bf16(after.T, act1, atol=3e-2, what="activation cache after the sparse step")
    assert_close_bf16(out1[0], ref, atol=6e-2, rtol=3e-2, what="sparse step output")


@pytest.mark.parametrize("N,fp8,offload", [(1000, False, False), (1003, False, False), (1000, True, False), (1003, False, True)])
def test_module_sparse_step_refreshes_the_stored_columns_only(dev, fresh_config, N, fp8, offload):
    """top_keys = 0.3: the columns in the stored indices are refreshed, every other cache column keeps its bits, and the output is the
    previous output plus delta @ fc2^T."""
    mlp, fc1, fc2, act, x0, x1 = _module(dev, fresh_config, N, 0.3, fp8, offload)
    out0, before, out1, after = _two_steps(mlp, x0, x1, offload)
    inds, counts = mlp.storage.get_indices()[0], mlp.storage.get_counts()[0]
    G = (N + BM - 1) // BM
    assert inds.shape == (G, before.shape[0]) and counts.shape == (G,)
    with torch.no_grad():
        act1 = act(fc1(x1))[0]
    for g in range(G):
        rows = slice(g * BM, min(N, (g + 1) * BM))
        n = int(counts[g])
        assert 0 < n < before.shape[0]
        cols = inds[g, :n].long()                 # (the entries past the count are not written by the index kernel: the complement is built here)
        assert int(cols.min()) >= 0 and int(cols.max()) < before.shape[0] and cols.unique().numel() == n
        keep = torch.ones(before.shape[0], dtype=torch.bool, device=cols.device)
        keep[cols] = False
        rest = keep.nonzero().flatten()
        assert_close_bf16(after[cols][:, rows].T, act1[rows][:, cols], atol=3e-2, what=f"group {g}: refreshed cache columns")
        assert torch.equal(after[rest][:, rows], before[rest][:, rows]), f"group {g}: a column outside the stored indices changed"
    delta = after.float() - before.float()                       # [F, N]: exactly the bf16 deltas where a column was refreshed, 0 elsewhere
    want = out0[0].float() + delta.T @ fc2.weight.float().T
    assert_close_bf16(out1[0], want, atol=6e-2, rtol=3e-2, what="sparse step output vs previous output + delta @ fc2^T")
