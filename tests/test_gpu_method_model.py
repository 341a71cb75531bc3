"""SparseDiffAttn / SparseDiffMlp on the device against the fp64 models of tests/method_model.py (run on the device too), over schedules
with inputs that change from step to step, layer to layer and model invocation to model invocation, driven by the integration protocol
(load_async_wait, load_async of the next layer, the call, complete_cur_layer): every route x the AMD switches on / off x the residency
set-ups.  After every call: the output, the stored state and the selection (method_model.AttnChecker / MlpChecker).  The bounds are the
floors tests/test_method_model_cpu.py pins on the CPU mirror times the margin; the same file proves that state defects are rejected."""
import contextlib
import os

import pytest
import torch

import method_model as mm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN_FLAGS = ("attn.out_cache", "attn.indices", "attn.counts", "attn.lse_constants")
MLP_FLAGS = ("mlp.out_cache", "mlp.indices", "mlp.counts", "mlp.sparse_act_T", "mlp.blockmean_mid_cache")
GENERAL_KERNELS = dict(attn_dense64=2, attn_colsum64=2, attn_csp96=2, attn_row_split=2)
# the scale fold of attn96.hip against plain exact attention, worst recorded in docs/TEST_SENSITIVITY.md; per gathered evaluation
FOLD_COST = 0.0143


def residency(flags, budget_gb):
    """name -> the offloading section: disabled; every field of the module through the host with the library's pinned pool / torch's;
    flagged but kept resident; flagged with a budget that holds some layers' tensors and not the others'"""
    on = dict({f: True for f in flags}, global_disable_offloading=False, keep_resident_if_fits=False, native_host_pool=True)
    return {
        "disabled": dict(global_disable_offloading=True),
        "host, native pool": on,
        "host, torch pool": dict(on, native_host_pool=False),
        "kept resident": dict(on, keep_resident_if_fits=True),
        "partly resident": dict(on, keep_resident_if_fits=True, hbm_budget_gb=budget_gb),
    }


# one attention cache (layer, invocation) is 2 x 832 x 128 x 2 B = 0.43 MB, one MLP activation cache 1024 x 1024 x 2 B = 2.1 MB
ATTN_RESIDENCY = residency(ATTN_FLAGS, 1.2e-3)
MLP_RESIDENCY = residency(MLP_FLAGS, 3e-3)


@pytest.fixture()
def dev(fresh_config):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    assert torch.cuda.is_available()
    ot.gpu_tensors.clear()
    saved = ot._resident_bytes, ot._kept_offloaded_bytes
    ot._resident_bytes = ot._kept_offloaded_bytes = 0
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    ot.gpu_tensors.clear()
    ot._resident_bytes, ot._kept_offloaded_bytes = saved


@contextlib.contextmanager
def options(**kw):
    from chipmunk_amd import _native
    try:
        for name, value in kw.items():
            _native.set_option(name, value)
        yield
    finally:
        for name in kw:
            _native.set_option(name, 0)


def _assert_mixed_residency(chk):
    """the budget of the "partly resident" set-up really splits the stored tensors between HBM and the host"""
    fields = [flag.split(".", 1)[1] for flag in ATTN_FLAGS + MLP_FLAGS]
    holders = [h for m in chk.modules for h in (getattr(m.storage, f, None) for f in fields) if h is not None]
    assert any(h.is_resident() for h in holders) and any(h.needs_host_copy() for h in holders)


def _report(what, chk):
    print(f"{what}: " + ", ".join(f"{k[0]}/{k[1]} {v:.4f}" for k, v in sorted(chk.worst.items())) + f", selection shortfall {chk.shortfall:.5f}")


@pytest.mark.parametrize("res", list(ATTN_RESIDENCY))
@pytest.mark.parametrize("token_major", [False, True], ids=["head-major", "token-major"])
@pytest.mark.parametrize("amd_keys", [True, False], ids=["amd keys default", "reference sequence"])
@pytest.mark.parametrize("route", list(mm.ATTN_ROUTES))
def test_attention_modules_against_the_method_model(dev, route, amd_keys, token_major, res):
    """General kernels forced: the allowance is ROW_ERR_BOUND + top-key term per attention evaluation + 2^-8 per stored bf16 sum."""
    what = f"attn {route}, {'amd' if amd_keys else 'ref'}, {'tm' if token_major else 'hm'}, {res}"
    with options(**GENERAL_KERNELS):
        chk = mm.run_attn_route(route, dev, ROOT, amd_keys=amd_keys, token_major=token_major, offloading=ATTN_RESIDENCY[res],
                                eps=2 * mm.ATTN_SELECTION_SHORTFALL[route], what=what)
    _report(what, chk)
    assert ("output", "sparse") in chk.worst and ("cache", "mask") in chk.worst
    if res == "partly resident":
        _assert_mixed_residency(chk)
    if amd_keys and route != "flux" and res.startswith("host"):
        # the shipped default with the mask on the host: the module keeps the index rows and suppresses the mask's load.  The checker's
        # read-back of a fresh mask sets that flag again, so it was in force in EVERY sparse step of every layer and invocation
        assert 0 < chk.sparse_calls == chk.suppressed_sparse_steps, (chk.sparse_calls, chk.suppressed_sparse_steps)


@pytest.mark.parametrize("route", list(mm.ATTN_ROUTES))
def test_attention_modules_with_the_shipped_kernel_dispatch(dev, route):
    """attn96.hip may fold the scale into Q: its recorded cost against plain exact attention is added per gathered evaluation."""
    what = f"attn {route}, shipped dispatch"
    chk = mm.run_attn_route(route, dev, ROOT, offloading=ATTN_RESIDENCY["disabled"], eps=2 * mm.ATTN_SELECTION_SHORTFALL[route],
                            per_sparse_eval=FOLD_COST, what=what)
    _report(what, chk)


@pytest.mark.parametrize("res", list(MLP_RESIDENCY))
@pytest.mark.parametrize("amd_keys", [True, False], ids=["amd keys default", "reference sequence"])
@pytest.mark.parametrize("n", [1024, 1003])
@pytest.mark.parametrize("route", list(mm.MLP_ROUTES_GPU))
def test_mlp_modules_against_the_method_model(dev, route, n, amd_keys, res):
    """K = 256, F = 1024; 1003 tokens are a multiple of neither 128 nor 8 (ragged last group, pitched cache).  Route wan: two model
    invocations with different inputs; wan_fp8: the same with the fp8 GEMM1 (the model takes the module's quantised operands)."""
    fp8 = route == "wan_fp8"
    if fp8:
        a = torch.zeros(16, mm.MLP_K, device=dev).to(torch.float8_e4m3fn)
        b = torch.zeros(mm.MLP_F, mm.MLP_K, device=dev).to(torch.float8_e4m3fn)
        one = torch.ones((), device=dev)
        try:        # torch's own fp8 GEMM, called as F8Linear calls it: its support varies with the ROCm build; nothing of the project runs here
            torch._scaled_mm(a, b.T, scale_a=one, scale_b=one, bias=torch.zeros(mm.MLP_F, device=dev, dtype=torch.bfloat16),
                             out_dtype=torch.bfloat16, use_fast_accum=True)
        except (RuntimeError, NotImplementedError) as e:
            pytest.skip(f"torch._scaled_mm fp8 unavailable here: {e}")
    what = f"mlp {route}, n {n}, {'amd' if amd_keys else 'ref'}, {res}"
    chk = mm.run_mlp_route(route, n, dev, torch.nn.Linear, torch.nn.GELU(approximate="tanh"), floors=mm.MLP_FLOORS,
                           eps=2 * (mm.MLP_SELECTION_SHORTFALL_FP8 if fp8 else mm.MLP_SELECTION_SHORTFALL), fp8=fp8, what=what, offloading=MLP_RESIDENCY[res],
                           amd_keys=amd_keys)
    _report(what, chk)
    assert ("output", 3) in chk.worst
    if res == "partly resident":
        _assert_mixed_residency(chk)
