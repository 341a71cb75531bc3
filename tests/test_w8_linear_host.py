"""The weight-only fp8 linear layer for few rows without a GPU ("Weight-only forward for few rows"): the key
``mlp.w8_stream_rows`` defaults to 0; the C entry ``chipmunk_w8_linear`` is declared, exported and refuses bad arguments with a code and a
message before any launch; the wrapper refuses by ``ValueError``; the fake kernel gives shapes; the CPU path follows the fp64 model within
the sparse MLP's segment bound, and mutants of the definition do not; ``W8Linear.forward`` on CPU tensors is the widened path whatever the
key says; the compiled ``w8_linear_kernel`` instantiations have no VGPR spill and no scratch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import w8_linear_model as model
from helpers import MLP_SEG_BOUND, assert_segs_close, seg_rel_err
from mlp_w8_model import E4M3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAME = "chipmunk_w8_linear"


# ------------------------------------------------------------------------------------------------------------------ config
def test_the_key_defaults_to_zero_and_amd_key_serves_it(fresh_config):
    from chipmunk_amd.util import config as cfg
    assert cfg.AMD_EXTRA_KEYS["mlp.w8_stream_rows"] == 0 and cfg.BASE_CONFIG["mlp"]["w8_stream_rows"] == 0
    assert type(cfg.AMD_EXTRA_KEYS["mlp.w8_stream_rows"]) is int
    assert cfg.amd_key("mlp", "w8_stream_rows") == 0
    fresh_config["mlp"]["w8_stream_rows"] = 256
    assert cfg.amd_key("mlp", "w8_stream_rows") == 256
    del fresh_config["mlp"]["w8_stream_rows"]
    assert cfg.amd_key("mlp", "w8_stream_rows") == 0


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_entry():
    from chipmunk_amd import _native
    header = open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read()
    assert NAME in _native.SYMBOLS and hasattr(_native.lib(), NAME), f"{NAME} is not exported"
    decl = re.search(rf"\bint {NAME}\s*\(([^;]*)\);", header).group(1)
    assert re.sub(r"\s+", " ", decl) == ("const void *x, int64_t ldx, const void *w, const float *scale_b, int scale_n, const void *bias, void *y, "
                                        "int64_t ldy, int M, int K, int F, void *stream")
    assert re.search(r"#define CHIPMUNK_W8_LINEAR_MAX_M \(1 << 20\)", header)
    assert _native.lib().chipmunk_abi_version() == 1


def _entry():
    """call(**overrides) -> (code, message); no launch happens: every call below is refused"""
    from chipmunk_amd import _native
    lib, p, null = _native.lib(), ctypes.c_void_p(256), ctypes.c_void_p(0)
    i, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    lib.chipmunk_w8_linear.argtypes = [vp, i64, vp, vp, i, vp, vp, i64, i, i, i, vp]
    base = dict(x=p, ldx=128, w=p, s=p, sn=1, bias=null, y=p, ldy=256, M=34, K=128, F=256)

    def call(**kw):
        v = dict(base, **kw)
        return lib.chipmunk_w8_linear(v["x"], v["ldx"], v["w"], v["s"], v["sn"], v["bias"], v["y"], v["ldy"], v["M"], v["K"], v["F"],
                                      null), _native.last_error()
    return call


VP = ctypes.c_void_p
REFUSALS = ((dict(x=VP(0)), "null"), (dict(w=VP(0)), "null"), (dict(s=VP(0)), "null"), (dict(y=VP(0)), "null"),
            (dict(sn=0), "scale_n must be 1"), (dict(sn=2), "scale_n must be 1"), (dict(sn=128), "scale_n must be 1"),
            (dict(s=VP(258)), "4-byte aligned"),
            (dict(x=VP(264)), "16-byte aligned"), (dict(y=VP(264)), "16-byte aligned"), (dict(bias=VP(264)), "16-byte aligned"),
            (dict(w=VP(264)), "16-byte aligned"),
            (dict(ldx=132), "multiples of 8"), (dict(ldy=260), "multiples of 8"),
            (dict(ldx=120), "ldx >= K"), (dict(ldy=248), "ldy >= F"),
            (dict(K=96, ldx=96), "multiple of 64"), (dict(F=252, ldy=256), "multiple of 8"),
            (dict(M=0), "M >= 1"), (dict(M=-3), "M >= 1"), (dict(K=0), "K >= 64"), (dict(K=32), "K >= 64"), (dict(F=0), "F >= 8"), (dict(F=4), "F >= 8"),
            (dict(M=(1 << 20) + 1), "above the grid"))


def test_the_entry_refuses_bad_arguments_before_any_launch():
    call = _entry()
    for kw, text in REFUSALS:
        rc, msg = call(**kw)
        assert rc == 1 and text in msg and msg.startswith("w8_linear:"), (kw, rc, msg)
    rc, msg = call(sn=256, x=VP(0))                  # scale_n == F passes that check: the refusal is another one
    assert rc == 1 and "scale_n" not in msg


# ------------------------------------------------------------------------------------------------------------------ wrapper, fake kernel
def test_wrapper_refusals_by_message():
    from chipmunk_amd import ops
    bf16 = torch.bfloat16
    x, w8, s = torch.zeros(3, 64, dtype=bf16), torch.zeros(16, 64).to(E4M3), torch.ones(1)
    with pytest.raises(ValueError, match="weight must be a float8_e4m3fn"):
        ops.w8_linear(x, w8.to(bf16), s)
    with pytest.raises(ValueError, match="weight must be a float8_e4m3fn"):
        ops.w8_linear(x, w8[0], s)
    with pytest.raises(ValueError, match="x must be bfloat16"):
        ops.w8_linear(x.float(), w8, s)
    with pytest.raises(ValueError, match=r"x must be \[..., K\] with K = 64"):
        ops.w8_linear(x[:, :32], w8, s)
    with pytest.raises(ValueError, match="scale must be float32 with one element or F = 16"):
        ops.w8_linear(x, w8, torch.ones(3))
    with pytest.raises(ValueError, match="scale must be float32"):
        ops.w8_linear(x, w8, s.to(bf16))
    with pytest.raises(ValueError, match="bias must be bfloat16 with F = 16"):
        ops.w8_linear(x, w8, s, torch.zeros(8, dtype=bf16))
    with pytest.raises(ValueError, match="bias must be bfloat16"):
        ops.w8_linear(x, w8, s, torch.zeros(16))
    assert "w8_linear" in ops.__all__
    y = ops.w8_linear(torch.zeros(2, 5, 64, dtype=bf16), w8, torch.ones(16), torch.zeros(16, dtype=bf16))
    assert y.shape == (2, 5, 16) and y.dtype == bf16


def test_fake_kernel_traces_without_a_gpu_and_checks_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        bf16 = torch.bfloat16
        x, w, y = torch.empty(34, 128, dtype=bf16), torch.empty(512, 128, dtype=E4M3), torch.empty(34, 512, dtype=bf16)
        op = torch.ops.chipmunk.w8_linear
        for s in (torch.empty(1), torch.empty(512)):
            assert op(x, w, s, torch.empty(512, dtype=bf16), y) is None
            assert op(x, w, s, None, y) is None
        with pytest.raises(RuntimeError, match="float8_e4m3fn"):
            op(x, w.to(bf16), torch.empty(1), None, y)
        with pytest.raises(RuntimeError, match="one element, or \\[F\\]"):
            op(x, w, torch.empty(2), None, y)
        with pytest.raises(RuntimeError, match=r"y \[M, F\]"):
            op(x, w, torch.empty(1), None, y[:, :8])
        with pytest.raises(RuntimeError, match="bias must have F entries"):
            op(x, w, torch.empty(1), torch.empty(8, dtype=bf16), y)


# ------------------------------------------------------------------------------------------------------------------ the CPU path
def _runs(shape):
    c = model.case(*shape)
    for vec in (False, True):
        for hb in (False, True):
            yield c, vec, hb, (c["sv"] if vec else c["s1"]), (c["bias"] if hb else None)


@pytest.mark.parametrize("shape", model.SHAPES_HOST, ids=lambda s: "x".join(map(str, s)))
def test_cpu_path_against_the_fp64_model(shape):
    from chipmunk_amd import ops
    worst = 0.0
    for c, vec, hb, s, b in _runs(shape):
        got = ops.w8_linear(c["x"], c["w"], s, b)
        assert got.dtype == torch.bfloat16 and torch.equal(got, model.definition(c["x"], c["w"], s, b)), "the wrapper's CPU path is the definition"
        worst = max(worst, assert_segs_close(got, c["exact"][(vec, hb)], MLP_SEG_BOUND, f"w8_linear cpu {shape} vec={vec} bias={hb}",
                                             width=model.SEG_WIDTH))
    print(f"w8_linear cpu path {shape}: worst segment {worst:.4f} (floor {model.FLOOR_W8_LINEAR}, bound {MLP_SEG_BOUND:.4f})")
    assert worst <= model.FLOOR_W8_LINEAR, "the pinned floor no longer covers the CPU path"


def test_floor_constant_is_tight():
    worst = max(float(seg_rel_err(model.definition(c["x"], c["w"], s, b), c["exact"][(vec, hb)], model.SEG_WIDTH).max())
                for shape in model.SHAPES_HOST for c, vec, hb, s, b in _runs(shape))
    assert 0.75 * model.FLOOR_W8_LINEAR <= worst <= model.FLOOR_W8_LINEAR < MLP_SEG_BOUND, worst


def test_mutants_of_the_definition_miss_the_bound():
    """each mutant on the vector-scale, biased run of the three shapes with K >= 192: counted when its worst segment reaches twice the
    bound at every one of them; one that does not is reported and not counted"""
    counted, report = [], []
    for mutant in model.MUTANTS:
        errs = []
        for shape in model.SHAPES_HOST[1:]:
            c = model.case(*shape)
            got = model.definition(c["x"], c["w"], c["sv"], c["bias"], mutant=mutant)
            errs.append(float(seg_rel_err(got, c["exact"][(True, True)], model.SEG_WIDTH).max()))
        ok = min(errs) >= 2 * MLP_SEG_BOUND
        (counted if ok else report).append(mutant)
        print(f"mutant {mutant}: worst segment per shape {['%.4g' % e for e in errs]} -> {'counted' if ok else 'NOT counted'}")
    assert len(counted) >= 5, f"counted {counted}, not counted {report}"


# ------------------------------------------------------------------------------------------------------------------ W8Linear.forward
def _layer(scaling, bias=True):
    from chipmunk_amd.modules import W8Linear
    torch.manual_seed(3)
    return W8Linear.from_linear(torch.nn.Linear(128, 64, bias=bias).bfloat16(), scaling=scaling)


@pytest.mark.parametrize("scaling", ["tensor", "row"])
def test_key_off_is_the_widened_linear_bit_for_bit(fresh_config, scaling):
    q = _layer(scaling)
    x = torch.randn(2, 17, 128).bfloat16()
    assert fresh_config["mlp"]["w8_stream_rows"] == 0
    assert torch.equal(q(x), torch.nn.functional.linear(x, q.widened(), q.bias))


def test_key_on_with_cpu_tensors_still_takes_the_widened_path(fresh_config, monkeypatch):
    import chipmunk_amd.ops
    calls = []
    monkeypatch.setattr(chipmunk_amd.ops, "w8_linear", lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError("called")))
    q = _layer("row")
    x = torch.randn(34, 128).bfloat16()
    off = q(x)
    fresh_config["mlp"]["w8_stream_rows"] = 1024
    assert torch.equal(q(x), off) and torch.equal(off, torch.nn.functional.linear(x, q.widened(), q.bias))
    assert calls == []


# ------------------------------------------------------------------------------------------------------------------ compile audit
def test_kernel_instantiations_without_spills_or_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "w8_linear.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "chipmunk_amd", "csrc", "w8_linear.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    inst = re.compile(r"16w8_linear_kernelILi(\d+)ELi(\d+)ELi(\d+)EEE")         # w8_linear_kernel<MT, NT, D>
    seen = set()
    for block in text.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "w8_linear_kernel" not in name.group(1):
            continue
        m = inst.search(name.group(1))
        assert m, f"an unexpected instantiation: {name.group(1)}"
        mt, nt, d = int(m.group(1)), int(m.group(2)), int(m.group(3))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spill == 0 and sspill == 0 and scratch == 0, f"{name.group(1)}: {spill} VGPR / {sspill} SGPR spills, {scratch} bytes of scratch"
        assert lds == 2 * mt * 16 * 128, f"{name.group(1)}: static LDS {lds}: two stages of {mt * 16} rows x 128 bytes and nothing else"
        assert d % 2 == 0 and mt * 16 <= 128, "at most 128 rows per block"
        seen.add((mt, nt, d))
    assert seen == {(1, 1, 8), (2, 1, 8), (3, 1, 8), (4, 1, 8), (6, 1, 6), (8, 2, 4)}, f"w8_linear_kernel<MT, NT, D>: {sorted(seen)}"
