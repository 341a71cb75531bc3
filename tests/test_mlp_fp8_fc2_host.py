"""fp8 fc2 in the sparse MLP without a GPU ("fp8 fc2"): the C ABI lists ``chipmunk_csp_mlp_mm2_w8[_batched]`` and refuses bad
arguments with codes and messages; the compiled ``mm2_w8_kernel`` instantiations have no VGPR spills and no scratch; the config key
``mlp.fp8_fc2`` defaults to off and, when on, lets ``recursive_swap_linears`` swap ``fc2`` of a sparse image MLP and both modules take an
e4m3 ``F8Linear`` ``fc2``; every e4m3 byte widens to bf16 exactly."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_abi_lists_the_two_entries_and_refuses_bad_arguments():
    import ctypes
    from chipmunk_amd import _native
    header = open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read()
    for name in ("chipmunk_csp_mlp_mm2_w8", "chipmunk_csp_mlp_mm2_w8_batched"):
        assert name in _native.SYMBOLS and re.search(rf"\b{name}\s*\(", header)
        assert hasattr(_native.lib(), name), f"{name} is not exported"
    assert _native.lib().chipmunk_abi_version() == 1
    lib, p, null = _native.lib(), ctypes.c_void_p(16), ctypes.c_void_p(0)      # (no launch happens: every call below is refused)

    def call(a=p, b=p, s=p, c=p, inds=p, cnt=p, M=100, F=256, N2=64):
        return lib.chipmunk_csp_mlp_mm2_w8(a, b, s, c, inds, cnt, M, F, N2, null), _native.last_error()
    for kw, text in ((dict(a=null), "null"), (dict(b=null), "null"), (dict(s=null), "null"), (dict(c=null), "null"),
                     (dict(inds=null), "indices / counts"), (dict(cnt=null), "indices / counts"), (dict(M=0), "M must be positive"),
                     (dict(F=96), "multiple of 64"), (dict(N2=0), "multiple of 16"), (dict(N2=24), "multiple of 16"), (dict(N2=8), "multiple of 16"),
                     (dict(M=1 << 20, F=2048), "32-bit offsets"),              # M * F = 2^31
                     (dict(F=1 << 16, N2=1 << 15), "32-bit offsets"),          # F * N2 = 2^31 one-byte elements
                     (dict(M=1 << 16, N2=1 << 15), "32-bit offsets")):         # M * N2 = 2^31
        rc, msg = call(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)
    batched = lib.chipmunk_csp_mlp_mm2_w8_batched
    for B, text in ((0, "batch size"), (-1, "batch size"), (65536, "65535")):
        rc = batched(p, p, p, p, p, p, 100, 256, 64, B, null)
        assert rc == 1 and text in _native.last_error(), (B, _native.last_error())
    rc = batched(p, p, p, p, p, p, 129, 256, 64, 32768, null)                  # 2 groups x 32768 sequences
    assert rc == 1 and "65535" in _native.last_error()
    rc = batched(p, p, null, p, p, p, 100, 256, 64, 2, null)
    assert rc == 1 and "null" in _native.last_error()
    rc = batched(p, p, p, p, p, p, 100, 256, 24, 2, null)
    assert rc == 1 and "multiple of 16" in _native.last_error()


def test_fake_kernel_traces_without_a_gpu_and_checks_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        bf16 = torch.bfloat16
        a, w, c = torch.empty(2, 333, 512, dtype=bf16), torch.empty(512, 256, dtype=E4M3), torch.empty(2, 333, 256, dtype=bf16)
        inds, counts, s = torch.empty(2, 3, 512, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32), torch.empty(1)
        op = torch.ops.chipmunk.csp_mlp_mm2_w8
        assert op(a, w, s, inds, counts, c) is None and op(a[0], w, s, inds[0], counts[0], c[0]) is None
        with pytest.raises(RuntimeError, match="float8_e4m3fn"):
            op(a, w.to(bf16), s, inds, counts, c)
        with pytest.raises(RuntimeError, match="one-element float32"):
            op(a, w, torch.empty(2), inds, counts, c)
        with pytest.raises(RuntimeError, match="shape mismatch"):
            op(a, w, s, inds, counts, c[0])


# ------------------------------------------------------------------------------------------------------------------ compile audit
def test_mm2_w8_kernels_compile_without_spills_or_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "mlp.s"        # (as tests/test_mlp_glu_host.py)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "chipmunk_amd", "csrc", "mlp.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    # mm2_w8_kernel<256, 32, 4, 2, 8, BATCHED>: the shipped shape, single and batched
    shipped = re.compile(r"13mm2_w8_kernelILi256ELi32ELi4ELi2ELi8ELb([01])EEE")
    seen = set()
    for block in text.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "mm2_w8_kernel" not in name.group(1):
            continue
        m = shipped.search(name.group(1))
        assert m, f"an fp8-weight GEMM2 instantiation other than the shipped tile shape: {name.group(1)}"
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spill == 0 and scratch == 0, f"{name.group(1)}: {spill} VGPR spills, {scratch} bytes of scratch"
        assert lds == 0, "the ring is dynamic LDS"
        seen.add(int(m.group(1)))
    assert seen == {0, 1}, f"mm2_w8_kernel instantiations (batched): {sorted(seen)}"


# ------------------------------------------------------------------------------------------------------------------ exactness
def test_every_e4m3_byte_widens_to_bf16_exactly():
    """f(w): the bits condition of tests/test_gpu_mlp_mm2_w8.py rests on bf16(e4m3) being the same number, also times 2^-3"""
    b = torch.arange(256, dtype=torch.uint8)
    w = b.view(E4M3)
    finite = (b & 0x7F) != 0x7F
    assert int(finite.sum()) == 254 and torch.isnan(w[~finite].float()).all()
    w16 = w.to(torch.bfloat16)
    assert torch.equal(w16[finite].double(), w[finite].double())
    assert torch.equal(w16[finite].to(E4M3).view(torch.uint8), b[finite]), "bf16 -> e4m3 gives the byte back"
    assert torch.equal((w16[finite] * 2.0 ** -3).double(), w[finite].double() * 2.0 ** -3)
    assert w[finite].double().abs().max() == 448 and w[finite].double().abs()[w[finite].double() != 0].min() == 2.0 ** -9


# ------------------------------------------------------------------------------------------------------------------ config, modules
def lin(i, o):
    return torch.nn.Linear(i, o).bfloat16()


def f8(i, o, **kw):
    from chipmunk_amd.modules import F8Linear
    return F8Linear.from_linear(lin(i, o), **kw)


def test_the_key_defaults_to_off_and_amd_key_serves_it(fresh_config):
    from chipmunk_amd.util import config as cfg
    assert cfg.AMD_EXTRA_KEYS["mlp.fp8_fc2"] is False and cfg.BASE_CONFIG["mlp"]["fp8_fc2"] is False
    assert cfg.amd_key("mlp", "fp8_fc2") is False
    fresh_config["mlp"]["fp8_fc2"] = True
    assert cfg.amd_key("mlp", "fp8_fc2") is True
    del fresh_config["mlp"]["fp8_fc2"]          # a section copied from the reference does not carry the key: the one default
    assert cfg.amd_key("mlp", "fp8_fc2") is False


def _block():
    blk = torch.nn.Module()
    blk.img_mlp = torch.nn.Sequential(lin(64, 128), torch.nn.GELU(approximate="tanh"), lin(128, 64))
    blk.txt_mlp = torch.nn.Sequential(lin(64, 128), torch.nn.GELU(approximate="tanh"), lin(128, 64))
    return blk


def test_recursive_swap_linears_swaps_fc2_of_a_sparse_image_mlp_with_the_key_on(fresh_config, capsys):
    from chipmunk_amd.modules import F8Linear
    from chipmunk_amd.modules.mlp_fp8 import recursive_swap_linears
    assert fresh_config["mlp"]["is_enabled"]
    off = _block()
    recursive_swap_linears(off)
    assert isinstance(off.img_mlp[0], F8Linear) and not isinstance(off.img_mlp[2], F8Linear) and isinstance(off.txt_mlp[2], F8Linear)
    assert "skipping fc2 of sparse img mlp" in capsys.readouterr().out
    fresh_config["mlp"]["fp8_fc2"] = True
    on = _block()
    recursive_swap_linears(on)
    assert isinstance(on.img_mlp[2], F8Linear) and on.img_mlp[2].weight.dtype == E4M3 and isinstance(on.img_mlp[0], F8Linear)
    assert "skipping" not in capsys.readouterr().out
    e5 = _block()
    recursive_swap_linears(e5, float8_dtype=E5M2)          # e5m2 weights: GEMM2 does not read them, fc2 stays bf16
    assert not isinstance(e5.img_mlp[2], F8Linear) and e5.img_mlp[0].weight.dtype == E5M2


def test_both_modules_take_an_e4m3_fc2_with_the_key_on_and_refuse_it_with_the_key_off(fresh_config):
    """construction only: no operator runs"""
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.modules import SparseDiffGatedMlp, SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    counter, silu, gelu = LayerCounter(1, 1), torch.nn.SiLU(), torch.nn.GELU(approximate="tanh")
    fc2 = f8(256, 128, input_float8_dtype=E4M3)
    for make in (lambda: SparseDiffMlp(0, counter, lin(128, 256), gelu, fc2),
                 lambda: SparseDiffGatedMlp(0, counter, lin(128, 256), lin(128, 256), silu, fc2),
                 lambda: SparseDiffGatedMlp.from_fused(0, counter, lin(128, 512), silu, fc2)):
        with pytest.raises(ValueError, match="mlp.fp8_fc2") as e:
            make()
        assert "fc2 must stay bf16" in str(e.value)
    fresh_config["mlp"]["fp8_fc2"] = True
    mods = [SparseDiffMlp(0, counter, lin(128, 256), gelu, fc2),
            SparseDiffMlp(0, counter, f8(128, 256, input_float8_dtype=E4M3), gelu, fc2),
            SparseDiffGatedMlp(0, counter, lin(128, 256), lin(128, 256), silu, fc2),
            SparseDiffGatedMlp(0, counter, f8(128, 256, input_float8_dtype=E4M3), f8(128, 256, input_float8_dtype=E4M3), silu, fc2),
            SparseDiffGatedMlp.from_fused(0, counter, lin(128, 512), silu, fc2)]
    for m in mods:
        wT = m.fc2w_T[0] if isinstance(m, SparseDiffMlp) else m.fc2w_T
        assert wT.dtype == E4M3 and tuple(wT.shape) == (256, 128) and wT.is_contiguous()
        assert torch.equal(wT.view(torch.uint8), fc2.weight.data.view(torch.uint8).T)
    bad = f8(256, 128, float8_dtype=E5M2, input_float8_dtype=E4M3)
    for make in (lambda: SparseDiffMlp(0, counter, lin(128, 256), gelu, bad),
                 lambda: SparseDiffGatedMlp(0, counter, lin(128, 256), lin(128, 256), silu, bad)):
        with pytest.raises(ValueError, match="e5m2 weights are refused"):
            make()
    # a bf16 fc2 is what it was, key on or off
    assert SparseDiffMlp(0, counter, lin(128, 256), gelu, lin(256, 128)).fc2w_T[0].dtype == torch.bfloat16


def test_ops_wrapper_needs_the_scale_for_an_e4m3_weight():
    from chipmunk_amd.ops.mlp import csp_mlp_mm2
    a, w, c = torch.zeros(128, 64, dtype=torch.bfloat16), torch.zeros(64, 32).to(E4M3), torch.zeros(128, 32, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="fc2_scale"):
        csp_mlp_mm2(a, w, torch.zeros(1, 64, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), c)
