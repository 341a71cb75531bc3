"""Weight-only fp8 fc1 without a GPU ("Weight-only fc1"): the C ABI declares and exports ``chipmunk_csp_mlp_mm1_w8[_batched|_gm]``
and refuses bad arguments with a code and a message, before any launch; the fake kernel gives shapes; the compiled code has exactly six
``mm1_w8_kernel`` instantiations at one tile shape, without VGPR spills, scratch or static LDS, under an LDS request of at most 80 KiB;
``W8Linear`` quantises with power-of-two scales, widens exactly and survives a state-dict round trip; the key ``mlp.fp8_weight_only``
defaults to off and switches ``recursive_swap_linears``; the gated module refuses ``W8Linear`` projections; the ``fc1_scale`` argument rules."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from mlp_w8_model import E4M3, every_byte_weight, pow2_quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = ("chipmunk_csp_mlp_mm1_w8", "chipmunk_csp_mlp_mm1_w8_batched", "chipmunk_csp_mlp_mm1_w8_gm")


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_three_entries():
    from chipmunk_amd import _native
    header = open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read()
    for name in NAMES:
        assert name in _native.SYMBOLS and re.search(rf"\bint {name}\s*\(", header), name
        assert hasattr(_native.lib(), name), f"{name} is not exported"
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", header).group(1)
        assert re.search(r"const void \*b,\s*const float \*scale_b,\s*int scale_n,", decl), f"{name}: scale_b, scale_n behind the weight"


def _entries():
    """the three entries as call(**overrides) -> (code, message); no launch happens: every call below is refused"""
    from chipmunk_amd import _native
    lib, p, null = _native.lib(), ctypes.c_void_p(256), ctypes.c_void_p(0)
    i, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    lib.chipmunk_csp_mlp_mm1_w8.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]
    lib.chipmunk_csp_mlp_mm1_w8_batched.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i64, vp]
    lib.chipmunk_csp_mlp_mm1_w8_gm.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i64, vp]
    base = dict(a=p, b=p, s=p, sn=1, c=p, bias=null, cache=p, inds=p, cnt=p, M=100, K=128, F=256, ldc=104, act=0, upd=0)

    def single(**kw):
        v = dict(base, **kw)
        return lib.chipmunk_csp_mlp_mm1_w8(v["a"], v["b"], v["s"], v["sn"], v["c"], v["bias"], v["cache"], v["inds"], v["cnt"], v["M"], v["K"],
                                           v["F"], v["ldc"], v["act"], v["upd"], null), _native.last_error()

    def batched(B=2, bs=256 * 104, **kw):
        v = dict(base, **kw)
        return lib.chipmunk_csp_mlp_mm1_w8_batched(v["a"], v["b"], v["s"], v["sn"], v["c"], v["bias"], v["cache"], v["inds"], v["cnt"], v["M"],
                                                   v["K"], v["F"], v["ldc"], v["act"], v["upd"], B, bs, null), _native.last_error()

    def gm(B=1, bs=256 * 128, **kw):
        v = dict(base, **kw)
        return lib.chipmunk_csp_mlp_mm1_w8_gm(v["a"], v["b"], v["s"], v["sn"], v["c"], v["bias"], v["cache"], v["inds"], v["cnt"], v["M"], v["K"],
                                              v["F"], v["act"], v["upd"], B, bs, null), _native.last_error()
    return single, batched, gm


REFUSALS = ((dict(a=ctypes.c_void_p(0)), "null"), (dict(b=ctypes.c_void_p(0)), "null"), (dict(s=ctypes.c_void_p(0)), "null"),
            (dict(c=ctypes.c_void_p(0)), "null"), (dict(cache=ctypes.c_void_p(0)), "null"),
            (dict(sn=0), "scale_n must be 1"), (dict(sn=2), "scale_n must be 1"), (dict(sn=128), "scale_n must be 1"),
            (dict(s=ctypes.c_void_p(258)), "4-byte aligned"),
            (dict(K=96), "multiple of 64"), (dict(K=0), "multiple of 64"),
            (dict(upd=2), "update_cache must be 0 or 1"), (dict(upd=-1), "update_cache must be 0 or 1"),
            (dict(act=3), "unknown activation"), (dict(act=-1), "unknown activation"),
            # ... and what check_mm1 refuses for the bf16 form
            (dict(inds=ctypes.c_void_p(0)), "indices / counts"), (dict(cnt=ctypes.c_void_p(0)), "indices / counts"),
            (dict(M=0), "M must be positive"), (dict(F=96), "multiple of 64"))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_every_entry_refuses_bad_arguments_before_any_launch(which):
    call = _entries()[which]
    for kw, text in REFUSALS:
        rc, msg = call(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)
    rc, msg = call(sn=256)                  # scale_n == F passes that check: the next refusal is another one
    assert "scale_n" not in msg


def test_the_entries_own_refusals():
    single, batched, gm = _entries()
    rc, msg = single(ldc=96)
    assert rc == 1 and "ldc" in msg                                  # a pitch below M
    rc, msg = single(M=1 << 16, K=1 << 15, ldc=1 << 16)
    assert rc == 1 and "32-bit offsets" in msg
    for B, text in ((0, "batch size"), (-1, "batch size"), (65536, "65535")):
        for call in (batched, gm):
            rc, msg = call(B=B)
            assert rc == 1 and text in msg, (B, msg)
    rc, msg = batched(bs=8)
    assert rc == 1 and "stride" in msg
    rc, msg = gm(bs=8)
    assert rc == 1 and "stride" in msg


def test_wrapper_refusals_by_message():
    """the operator's own checks in front of the entry (no GPU: the device check comes first for CPU tensors, so the rules that can be
    reached without one are the wrappers' -- tests/test_gpu_mlp_w8.py reaches the rest)"""
    from chipmunk_amd.ops.mlp import mm1, mm1_scatter, mm1_w8, run_e2e
    bf16 = torch.bfloat16
    x, w8 = torch.zeros(128, 64, dtype=bf16), torch.zeros(64, 64).to(E4M3)
    packed, cache = torch.zeros(128, 64, dtype=bf16), torch.zeros(64, 128, dtype=bf16)
    inds, cnt, s = torch.zeros(1, 64, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.ones(())
    with pytest.raises(ValueError, match="unknown activation"):
        mm1_w8(x, w8, s, packed, None, cache, inds, cnt, act="relu")
    with pytest.raises(ValueError, match="fc1_scale.*float8_e4m3fn fc1w"):
        mm1(x, w8.to(bf16), packed, None, cache, inds, cnt, fc1_scale=s)
    with pytest.raises(ValueError, match="x must be bfloat16"):
        mm1(x.to(E4M3), w8, packed, None, cache, inds, cnt, fc1_scale=s)
    with pytest.raises(ValueError, match="scale_a must be None"):
        mm1(x, w8, packed, None, cache, inds, cnt, scale_a=s, fc1_scale=s)
    with pytest.raises(ValueError, match="scale_b must be None"):
        mm1(x, w8, packed, None, cache, inds, cnt, scale_b=s, fc1_scale=s)
    with pytest.raises(ValueError, match="fc1_scale must hold one number"):
        mm1_scatter(x, w8, packed, None, cache, inds, cnt, fc1_scale=torch.ones(3))
    out = torch.zeros(128, 32, dtype=bf16)
    with pytest.raises(ValueError, match="mm1_scale_a must be None"):
        run_e2e(x, w8, None, torch.zeros(64, 32, dtype=bf16), inds, cnt, cache, out, 0, mm1_scale_a=s, fc1_scale=s)
    with pytest.raises(ValueError, match="mm1_scale_b must be None"):
        run_e2e(x, w8, None, torch.zeros(64, 32, dtype=bf16), inds, cnt, cache, out, 0, mm1_scale_b=s, fc1_scale=s)
    with pytest.raises(ValueError, match="run_e2e: fc1_scale.*fc1w is torch.bfloat16"):
        run_e2e(x, w8.to(bf16), None, torch.zeros(64, 32, dtype=bf16), inds, cnt, cache, out, 0, fc1_scale=s)
    # without fc1_scale an e4m3 fc1w under a bf16 x is refused as it always was
    with pytest.raises(AssertionError):
        mm1(x, w8, packed, None, cache, inds, cnt)


def test_fake_kernel_traces_without_a_gpu_and_checks_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        bf16 = torch.bfloat16
        a, w, c = torch.empty(2, 333, 128, dtype=bf16), torch.empty(512, 128, dtype=E4M3), torch.empty(2, 333, 512, dtype=bf16)
        cache, bias = torch.empty(2, 512, 333, dtype=bf16), torch.empty(512, dtype=bf16)
        inds, counts = torch.empty(2, 3, 512, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32)
        op = torch.ops.chipmunk.csp_mlp_mm1_w8
        for s in (torch.empty(1), torch.empty(512)):
            assert op(a, w, s, c, bias, cache, inds, counts, "silu", True) is None
            assert op(a[0], w, s, c[0], None, cache[0], inds[0], counts[0], "gelu", False) is None
        with pytest.raises(RuntimeError, match="float8_e4m3fn"):
            op(a, w.to(bf16), torch.empty(1), c, bias, cache, inds, counts, "silu", True)
        with pytest.raises(RuntimeError, match="one element, or \\[F\\]"):
            op(a, w, torch.empty(2), c, bias, cache, inds, counts, "silu", True)
        with pytest.raises(RuntimeError, match="c must be"):
            op(a, w, torch.empty(1), c[0], bias, cache, inds, counts, "silu", True)
        with pytest.raises(RuntimeError, match="unknown activation"):
            op(a, w, torch.empty(1), c, bias, cache, inds, counts, "relu", True)


# ------------------------------------------------------------------------------------------------------------------ compile audit
def test_six_kernels_at_one_tile_shape_without_spills_scratch_or_static_lds(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "mlp.s"        # (as tests/test_mlp_fp8_fc2_host.py)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "chipmunk_amd", "csrc", "mlp.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    # mm1_w8_kernel<BN, BK, NST, WPS, ACT, BATCHED>
    inst = re.compile(r"13mm1_w8_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi([012])ELb([01])EEE")
    seen, shapes = set(), set()
    for block in text.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "mm1_w8_kernel" not in name.group(1):
            continue
        m = inst.search(name.group(1))
        assert m, f"an unexpected weight-only GEMM1 instantiation: {name.group(1)}"
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spill == 0 and scratch == 0, f"{name.group(1)}: {spill} VGPR spills, {scratch} bytes of scratch"
        assert lds == 0, "the ring is dynamic LDS"
        shapes.add(tuple(int(v) for v in m.groups()[:4]))
        seen.add((int(m.group(5)), int(m.group(6))))
    assert seen == {(act, b) for act in (0, 1, 2) for b in (0, 1)}, f"mm1_w8_kernel instantiations (act, batched): {sorted(seen)}"
    assert len(shapes) == 1, f"more than one tile shape: {sorted(shapes)}"
    bn, bk, nst, wps = next(iter(shapes))
    # the launcher's request: NST stages of 128 bf16 A rows and BN e4m3 B rows of one k step, + 16 bytes per 32 B rows (the shifted pieces)
    request = nst * (128 * bk * 2 + bn * bk + bn // 32 * 16)
    src = open(os.path.join(ROOT, "chipmunk_amd", "csrc", "mlp.hip")).read()
    launcher = src[src.index("int launch_mm1_w8_kernel("):]
    launcher = launcher[: launcher.index("CM_LAUNCH_CHECK")]
    assert re.search(rf"constexpr int BN = {bn}, BK = {bk}, NST = {nst}, WPS = {wps};", launcher), "the launcher's shape is the kernels'"
    assert "constexpr int LDS = NST * (BM * BK * 2 + BN * BK + BN / 32 * 16);" in launcher and "static_assert(LDS <= 80 * 1024" in launcher
    assert request <= 80 * 1024 and wps == 2, f"LDS request {request} bytes: two workgroups must share a CU"
    # its own launcher: the line the form audit counts stays what it was
    assert len(re.findall(r"launch_mm1_variant<128, 64, 2, 2, FP8, 4, BATCHED, GLU, [012], RS>", src)) == 3


# ------------------------------------------------------------------------------------------------------------------ W8Linear
def lin(i, o, bias=True, seed=0):
    torch.manual_seed(seed)
    m = torch.nn.Linear(i, o, bias=bias).bfloat16()
    with torch.no_grad():       # rows of very different size: the per-row scales differ
        m.weight.mul_(torch.logspace(-3, 2, o).unsqueeze(1).to(torch.bfloat16))
    return m


@pytest.mark.parametrize("scaling", ["tensor", "row"])
def test_w8linear_quantises_with_power_of_two_scales_and_widens_exactly(scaling):
    from chipmunk_amd.modules import W8Linear
    src = lin(96, 40)
    q = W8Linear.from_linear(src, scaling=scaling)
    assert q.weight_only is True and q.scaling == scaling
    assert q.weight.dtype == E4M3 and tuple(q.weight.shape) == (40, 96) and q.scale_reciprocal.dtype == torch.float32
    assert tuple(q.scale_reciprocal.shape) == ((40,) if scaling == "row" else ())
    mant, _ = torch.frexp(q.scale_reciprocal)
    assert (mant == 0.5).all(), "scales are powers of two"
    w8, recip = pow2_quantize(src.weight.data, scaling)
    assert torch.equal(q.scale_reciprocal, recip) and torch.equal(q.weight.data.view(torch.uint8), w8.view(torch.uint8))
    # no amax maps below 224 or above 448
    wd = src.weight.data.double()
    amax = wd.abs().amax(dim=1) if scaling == "row" else wd.abs().amax()
    mapped = amax / q.scale_reciprocal.double()
    assert (mapped > 224).all() and (mapped <= 448).all(), mapped
    # the widened product is exact, and it is what forward multiplies by
    s = q.scale_reciprocal.unsqueeze(1) if scaling == "row" else q.scale_reciprocal
    wide = q.widened()
    assert wide.dtype == torch.bfloat16 and torch.equal(wide.float(), q.weight.float() * s)
    x = torch.randn(3, 7, 96).bfloat16()
    assert torch.equal(q(x), torch.nn.functional.linear(x, wide, src.bias))
    assert not any(t.dtype == torch.bfloat16 and t.shape == q.weight.shape for t in list(q.buffers()) + list(q.__dict__.values())
                   if isinstance(t, torch.Tensor)), "a widened copy must not be kept"
    assert sum(p.numel() * p.element_size() for p in q.parameters() if p.ndim == 2) == 40 * 96


def test_w8linear_every_byte_and_zero_rows():
    from chipmunk_amd.modules import W8Linear
    w = every_byte_weight(8, 256, seed=3).to(torch.bfloat16) * 2.0 ** -6
    w[3] = 0                                   # an all-zero row: scale 1
    src = torch.nn.Linear(256, 8, bias=False).bfloat16()
    src.weight.data = w
    q = W8Linear.from_linear(src, scaling="row")
    assert q.bias is None and float(q.scale_reciprocal[3]) == 1.0 and (q.weight[3].float() == 0).all()
    assert torch.equal(q.widened().float(), w.float()), "e4m3 values times a power of two come back exactly"


@pytest.mark.parametrize("scaling", ["tensor", "row"])
def test_w8linear_state_dict_round_trip(scaling):
    from chipmunk_amd.modules import W8Linear
    q = W8Linear.from_linear(lin(64, 24, seed=2), scaling=scaling)
    sd = q.state_dict()
    assert set(sd) == {"weight", "bias", "scale_reciprocal"} and sd["weight"].dtype == E4M3
    r = W8Linear(64, 24, bias=True, scaling=scaling)
    r.load_state_dict(sd)
    assert torch.equal(r.weight.data.view(torch.uint8), q.weight.data.view(torch.uint8)) and torch.equal(r.scale_reciprocal, q.scale_reciprocal)
    assert torch.equal(r.bias, q.bias)
    x = torch.randn(5, 64).bfloat16()
    assert torch.equal(r(x), q(x))


# ------------------------------------------------------------------------------------------------------------------ config, modules
def test_the_key_defaults_to_off_and_amd_key_serves_it(fresh_config):
    from chipmunk_amd.util import config as cfg
    assert cfg.AMD_EXTRA_KEYS["mlp.fp8_weight_only"] is False and cfg.BASE_CONFIG["mlp"]["fp8_weight_only"] is False
    assert cfg.amd_key("mlp", "fp8_weight_only") is False
    fresh_config["mlp"]["fp8_weight_only"] = True
    assert cfg.amd_key("mlp", "fp8_weight_only") is True
    del fresh_config["mlp"]["fp8_weight_only"]
    assert cfg.amd_key("mlp", "fp8_weight_only") is False


def _block():
    plain = lambda i, o: torch.nn.Linear(i, o).bfloat16()      # noqa: E731
    blk = torch.nn.Module()
    blk.img_mlp = torch.nn.Sequential(plain(64, 128), torch.nn.GELU(approximate="tanh"), plain(128, 64))
    blk.txt_mlp = torch.nn.Sequential(plain(64, 128), torch.nn.GELU(approximate="tanh"), plain(128, 64))
    blk.img_mod = torch.nn.Linear(64, 64).bfloat16()
    return blk


def test_recursive_swap_linears_with_the_key_on_and_off(fresh_config, capsys):
    from chipmunk_amd.modules import F8Linear, W8Linear
    from chipmunk_amd.modules.mlp_fp8 import recursive_swap_linears
    assert fresh_config["mlp"]["is_enabled"]
    off = _block()
    recursive_swap_linears(off)
    assert isinstance(off.img_mlp[0], F8Linear) and isinstance(off.img_mlp[2], torch.nn.Linear) and isinstance(off.txt_mlp[2], F8Linear)
    assert not any(isinstance(m, W8Linear) for m in off.modules())
    fresh_config["mlp"]["fp8_weight_only"] = True
    capsys.readouterr()
    on = _block()
    recursive_swap_linears(on)
    assert isinstance(on.img_mlp[0], W8Linear) and isinstance(on.txt_mlp[0], W8Linear) and isinstance(on.txt_mlp[2], W8Linear)
    assert type(on.img_mlp[2]) is torch.nn.Linear and "skipping fc2 of sparse img mlp" in capsys.readouterr().out      # the fp8_fc2 rule
    assert type(on.img_mod) is torch.nn.Linear                                                                       # the same exclusions
    assert not any(isinstance(m, F8Linear) for m in on.modules())
    fresh_config["mlp"]["fp8_fc2"] = True
    fresh_config["mlp"]["fp8_scaling"] = "row"
    both = _block()
    recursive_swap_linears(both)
    assert isinstance(both.img_mlp[2], W8Linear) and both.img_mlp[2].scaling == "tensor" and both.img_mlp[2].scale_reciprocal.numel() == 1
    assert both.img_mlp[0].scaling == "row" and tuple(both.img_mlp[0].scale_reciprocal.shape) == (128,)
    with pytest.raises(ValueError, match="fp8_weight_only"):
        recursive_swap_linears(_block(), float8_dtype=torch.float8_e5m2)


def test_modules_take_and_refuse_w8linear(fresh_config):
    """construction only: no operator runs"""
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.modules import SparseDiffGatedMlp, SparseDiffMlp, W8Linear
    from chipmunk_amd.util.layer_counter import LayerCounter
    plain = lambda i, o: torch.nn.Linear(i, o).bfloat16()      # noqa: E731
    w8 = lambda i, o, **kw: W8Linear.from_linear(plain(i, o), **kw)      # noqa: E731
    counter, silu, gelu = LayerCounter(1, 1), torch.nn.SiLU(), torch.nn.GELU(approximate="tanh")
    for scaling in ("tensor", "row"):
        m = SparseDiffMlp(0, counter, w8(128, 256, scaling=scaling), gelu, plain(256, 128))
        assert m.fc1[0].weight_only and m.fc2w_T[0].dtype == torch.bfloat16
    with pytest.raises(ValueError, match="fc2 must stay bf16"):
        SparseDiffMlp(0, counter, w8(128, 256), gelu, w8(256, 128))
    for make in (lambda: SparseDiffGatedMlp(0, counter, w8(128, 256), w8(128, 256), silu, plain(256, 128)),
                 lambda: SparseDiffGatedMlp(0, counter, w8(128, 256), plain(128, 256), silu, plain(256, 128)),
                 lambda: SparseDiffGatedMlp.from_fused(0, counter, w8(128, 512), silu, plain(256, 128))):
        with pytest.raises(ValueError, match="only the ungated GEMM1 has a weight-only form"):
            make()
    fresh_config["mlp"]["fp8_fc2"] = True
    fc2 = w8(256, 128)
    m = SparseDiffMlp(0, counter, w8(128, 256, scaling="row"), gelu, fc2)
    assert m.fc2w_T[0].dtype == E4M3 and torch.equal(m.fc2w_T[0].view(torch.uint8), fc2.weight.data.view(torch.uint8).T)
    g = SparseDiffGatedMlp(0, counter, plain(128, 256), plain(128, 256), silu, fc2)       # a W8Linear fc2 under the gated module as well
    assert g.fc2w_T.dtype == E4M3
    with pytest.raises(ValueError, match="row-scaled fc2"):
        SparseDiffMlp(0, counter, plain(128, 256), gelu, w8(256, 128, scaling="row"))
