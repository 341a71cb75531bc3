"""Batches through the full-size launches and through the SparseDiffMlp module.

Full size, one launch per kernel (GEMM1 with its scatter-add, then GEMM2) over all B sequences: the batched launch bit for bit against the
per-sequence launches of today's 2-D operators, and the last group of the last sequence against fp32 torch.  FLUX (bf16, B = 4), the
Wan2.1 cond / uncond pair (fp8, B = 2) and HunyuanVideo (bf16, B = 2: B * M * F = 2.93e9 > 2^31, so a batch base formed in 32 bits fails).

Module: B = 2, a full step and two sparse steps.  Each sparse step is replayed per sequence through the B = 1 operators on clones of that
sequence's slices of the state stored before it, with fc1(block_mean(x)) and the quantised input taken from the batched run (so the dense
GEMM and the quantisation are common to both sides): the module's output and every stored tensor must equal the replay bit for bit."""
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


@pytest.mark.parametrize("name,B,M,K,F,N2,fp8", [("flux", 4, 4352, 3072, 12288, 3072, False), ("wan", 2, 32760, 1536, 8960, 1536, True),
                                                 ("hunyuan", 2, 119056, 3072, 12288, 3072, False)])
def test_full_size_batched_gemm1_scatter_then_gemm2(dev, name, B, M, K, F, N2, fp8):
    G = (M + BM - 1) // BM
    assert M % 8 == 0
    # the 32-bit-offset conditions hold per sequence (HunyuanVideo: not for the batch)
    assert M * K < 2 ** 31 and F * K < 2 ** 31 and F * M < 2 ** 31 and M * F < 2 ** 31 and F * N2 < 2 ** 31
    assert name != "hunyuan" or B * M * F > 2 ** 31
    g_ = torch.Generator(device=dev).manual_seed(M + B)
    x = torch.randn(B, M, K, device=dev, generator=g_) * 0.5
    w = torch.randn(F, K, device=dev, generator=g_) * 0.05
    ra = rb = None
    if fp8:
        sa, sb = 448.0 / x.abs().max(), 448.0 / w.abs().max()
        a, w1 = (x * sa).to(torch.float8_e4m3fn), (w * sb).to(torch.float8_e4m3fn)
        ra, rb = (1.0 / sa).reshape(1).float(), (1.0 / sb).reshape(1).float()
    else:
        a, w1 = x.to(torch.bfloat16), w.to(torch.bfloat16)
    del x, w
    bias = (torch.randn(F, device=dev, generator=g_) * 0.2).to(torch.bfloat16)
    w2T = (torch.randn(F, N2, device=dev, generator=g_) * 0.03).to(torch.bfloat16)
    out0 = torch.empty(B, M, N2, dtype=torch.bfloat16, device=dev).normal_(generator=g_).mul_(0.5)
    cache_buf = torch.empty(B, F + 1, M, dtype=torch.bfloat16, device=dev)       # ldc == M, one canary row behind every sequence
    cache_buf.normal_(generator=g_).mul_(0.3)
    cache_buf[:, F] = 7.0
    inds = torch.stack([torch.rand(G, F, device=dev, generator=g_).argsort(dim=1).to(torch.int32) for _ in range(B)])
    counts = (torch.randint(10, 16, (B, G), device=dev, generator=g_) * 256).to(torch.int32)      # as tests/test_gpu_mlp_ragged_e2e.py
    counts[:, G // 3] = 0

    def run(batched):
        cb = cache_buf.clone()
        cache = cb[:, :F]
        c_buf = torch.full((B * M + BM, F), 7.0, dtype=torch.bfloat16, device=dev)
        out_buf = torch.full((B * M + BM, N2), 7.0, dtype=torch.bfloat16, device=dev)
        c, out = c_buf[:B * M].view(B, M, F), out_buf[:B * M].view(B, M, N2)
        out.copy_(out0)
        ops = torch.ops.chipmunk
        for b in ([slice(None)] if batched else range(B)):      # one launch per kernel, or one per kernel and sequence
            if fp8:
                ops.csp_mlp_mm1_fp8_scatter(a[b], w1, c[b], bias, cache[b], inds[b], counts[b], ra, rb)
            else:
                ops.csp_mlp_mm1_scatter(a[b], w1, c[b], bias, cache[b], inds[b], counts[b])
            ops.csp_mlp_mm2(c[b], w2T, inds[b], counts[b], out[b])
        torch.cuda.synchronize()
        return cb, c_buf, out_buf

    ref = run(False)
    got = run(True)
    for what, x, y in zip(("cache", "packed deltas", "mma_c"), got, ref):
        same = torch.equal(x.view(torch.int16), y.view(torch.int16))
        assert same, f"{name}: {what} of the batched launch differ from the per-sequence launches"
    cb, c_buf, out_buf = got
    del ref
    assert (c_buf[B * M:] == 7.0).all() and (out_buf[B * M:] == 7.0).all() and (cb[:, F] == 7.0).all(), "a canary row changed"
    # the last group of the last sequence against fp32 torch
    b, g = B - 1, G - 1
    c, out, cache = c_buf[:B * M].view(B, M, F)[b], out_buf[:B * M].view(B, M, N2)[b], cb[b, :F]
    rows = slice(g * BM, M)
    n = int(counts[b, g])
    assert n > 0 and (c[rows, n:] == 7.0).all(), f"{name}: packed columns past the count written"
    cols, rest = inds[b, g, :n].long(), inds[b, g, n:].long()
    old = cache_buf[b, :F, rows]
    assert torch.equal(cache[:, rows][rest], old[rest]), f"{name}: unselected cache columns changed"
    if fp8:
        acc = (a[b, rows].float() @ w1[cols].float().T) * ra * rb + bias[cols].float()
        act = torch.nn.functional.gelu(acc, approximate="tanh").to(torch.bfloat16).float()
        want = (act - old[cols].float().T).to(torch.bfloat16)
        tol = dict(atol=3e-2, rtol=3e-2)
    else:
        act = torch.nn.functional.gelu(a[b, rows].float() @ w1[cols].float().T + bias[cols].float(), approximate="tanh")
        want = act - old[cols].float().T
        tol = {}
    assert_close_bf16(c[rows, :n], want, what=f"{name} GEMM1, last group of sequence {b} vs fp32 torch", **tol)
    new = (old[cols].float() + c[rows, :n].float().T).to(torch.bfloat16)
    assert torch.equal(cache[:, rows][cols], new), f"{name}: cache != bf16(cache + delta)"
    prod = (c[rows, :n].float() @ w2T[cols].float()).to(torch.bfloat16)
    assert_close_bf16(out[rows], prod.float() + out0[b, rows].float(), what=f"{name} GEMM2, last group of sequence {b} vs fp32 torch")


# ------------------------------------------------------------------------------------------------ the module
class Recorder:
    """Stands in for the module's fc1: records what the dense fc1 call returns (fc1(block_mean(x))) and what quantize_input returns, so
    that the replay uses the batched run's values."""

    def __init__(self, inner):
        self.__dict__["inner"] = inner
        self.__dict__["dense"] = []
        self.__dict__["quant"] = []

    def __call__(self, x):
        y = self.inner(x)
        self.dense.append(y.clone())
        return y

    def quantize_input(self, x):
        q = self.inner.quantize_input(x)
        self.quant.append((q.clone(), self.inner.input_scale_reciprocal.clone()))
        return q

    def __getattr__(self, name):
        return getattr(self.inner, name)


def _module(dev, cfg, B, N, top_keys, fp8, offload):
    from chipmunk_amd.modules import SparseDiffMlp, F8Linear
    from chipmunk_amd.util.layer_counter import LayerCounter
    cfg["offloading"]["global_disable_offloading"] = not offload
    if offload:
        cfg["offloading"]["mlp.sparse_act_T"] = True
        cfg["offloading"]["keep_resident_if_fits"] = False
    cfg["mlp"].update(dict(top_keys=top_keys, random_keys=0.0, full_step_every=4, block_mask_cache=2, first_n_dense_layers=0,
                           counts_multiple_of=256))
    torch.manual_seed(N + B)
    K, F = 256, 1024
    fc1 = torch.nn.Linear(K, F, device=dev, dtype=torch.bfloat16)
    if fp8:
        fc1 = F8Linear.from_linear(fc1, input_float8_dtype=torch.float8_e4m3fn)
    fc2 = torch.nn.Linear(F, K, device=dev, dtype=torch.bfloat16)
    act = torch.nn.GELU(approximate="tanh")
    mlp = SparseDiffMlp(0, LayerCounter(1, 1), fc1, act, fc2, 6)
    xs = [torch.randn(B, N, K, device=dev, dtype=torch.bfloat16)]
    for _ in range(2):
        xs.append(xs[-1] + 0.3 * torch.randn_like(xs[0]))
    if fp8:
        try:                               # torch._scaled_mm support varies with the ROCm build (as in tests/test_gpu_mlp.py's fp8 module test)
            with torch.no_grad():
                fc1(xs[0])
        except (RuntimeError, NotImplementedError) as e:
            pytest.skip(f"torch._scaled_mm fp8 unavailable here: {e}")
    return mlp, fc1, fc2, act, xs


def _reload(mlp, offload):
    if offload:
        mlp.storage.load_async()
        mlp.storage.load_async_wait()


def _snapshot(mlp):
    st = mlp.storage
    return dict(act_T=st.get_sparse_act_T().clone(), out=st.get_out_cache().clone(), bm=st.get_blockmean_mid_cache().clone())


@pytest.mark.parametrize("top_keys", [1.0, 0.3])
@pytest.mark.parametrize("offload", [False, True], ids=["resident", "offloaded"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("N", [1000, 1003])
def test_module_batch_of_two_equals_the_per_sequence_replay(dev, fresh_config, N, fp8, offload, top_keys):
    from chipmunk_amd import ops
    from chipmunk_amd.util.config import amd_key
    cfg = fresh_config
    B = 2
    mlp, fc1, fc2, act, xs = _module(dev, cfg, B, N, top_keys, fp8, offload)
    mcfg = cfg["mlp"]
    assert mcfg["bm"] == mcfg["mbm"] and amd_key("mlp", "fused_topk_delta"), "the replay below is the module's default operator sequence"
    Fdim, ld, G = fc1.out_features, (N + 7) // 8 * 8, (N + BM - 1) // BM
    with torch.no_grad():
        out0 = mlp(xs[0])
        assert out0.shape == (B, N, fc2.out_features)
        rec = Recorder(fc1)
        mlp.fc1[0] = rec
        for step in (1, 2):
            x = xs[step]
            _reload(mlp, offload)
            snap = _snapshot(mlp)
            assert snap["act_T"].shape == (B, Fdim, ld) and snap["out"].shape == (B, N, fc2.out_features) and snap["bm"].shape == (B, G, Fdim)
            assert (snap["act_T"][..., N:] == 0).all() or step > 1
            out = mlp(x).clone()
            torch.cuda.synchronize()
            st = mlp.storage
            got = dict(act_T=st.get_sparse_act_T(), out=st.get_out_cache(), bm=st.get_blockmean_mid_cache(), inds=st.get_indices(), counts=st.get_counts())
            assert got["inds"].shape == (B, G, Fdim) and got["counts"].shape == (B, G) and got["act_T"].shape == (B, Fdim, ld)
            assert torch.equal(out, got["out"])
            bmfc1 = rec.dense[-1]                       # fc1(block_mean(x)) of the batched run: [B, G, F]
            assert bmfc1.shape == (B, G, Fdim)
            for b in range(B):
                # the sparse step's operator sequence through the B = 1 operators, on clones of sequence b's slices
                bm_b = snap["bm"][b:b + 1].clone()
                inds_b = torch.empty(1, G, Fdim, dtype=torch.int32, device=dev)
                counts_b = torch.empty(1, G, dtype=torch.int32, device=dev)
                torch.ops.chipmunk.topk_delta_indices(bmfc1[b:b + 1].contiguous(), bm_b, inds_b, counts_b, 1 - mcfg["top_keys"],
                                                      mcfg["counts_multiple_of"], mcfg["random_keys"])
                act_b, out_b = snap["act_T"][b].clone(), snap["out"][b].clone()
                scale_a = scale_b = None
                xb = x[b]
                if fp8:
                    xq, scale_a = rec.quant[-1]
                    xb, scale_b = xq[b], fc1.scale_reciprocal
                ops.mlp(x=xb, fc1w=fc1.weight.data, fc1b=fc1.bias.data, fc2w_T=mlp.fc2w_T[0], indices=inds_b[0], counts=counts_b[0],
                        sparse_act_T=act_b[:, :N], cached_out=out_b, num_sms_scatter_add=6, mm1_scale_a=scale_a, mm1_scale_b=scale_b)
                torch.cuda.synchronize()
                what = f"step {step}, sequence {b}"
                assert torch.equal(got["counts"][b], counts_b[0]), f"{what}: counts"
                for g in range(G):
                    n = int(counts_b[0, g])
                    assert torch.equal(got["inds"][b, g, :n], inds_b[0, g, :n]), f"{what}: indices of group {g}"
                assert torch.equal(got["bm"][b].view(torch.int16), bm_b[0].view(torch.int16)), f"{what}: block means"
                assert torch.equal(got["act_T"][b].view(torch.int16), act_b.view(torch.int16)), f"{what}: activation cache"
                assert torch.equal(got["out"][b].view(torch.int16), out_b.view(torch.int16)), f"{what}: output"
                if top_keys == 1.0:
                    assert (counts_b == Fdim).all()
            if top_keys == 1.0:     # every column refreshed: the dense MLP on the new input (tolerances of the ragged module test)
                act1 = act(fc1(x))
                ref = fc2(act1)
                assert_close_bf16(got["act_T"][..., :N].transpose(1, 2), act1, atol=3e-2, what=f"step {step}: activation cache")
                assert_close_bf16(out, ref, atol=6e-2, rtol=3e-2, what=f"step {step}: output vs the dense MLP")


def test_module_refuses_a_sparse_step_at_another_batch_size(dev, fresh_config):
    mlp, fc1, fc2, act, xs = _module(dev, fresh_config, 2, 1000, 0.3, False, False)
    with torch.no_grad():
        mlp(xs[0])
        with pytest.raises(RuntimeError, match="batch size 2 with 1000 tokens"):
            mlp(torch.cat([xs[1], xs[1][:1]]))
