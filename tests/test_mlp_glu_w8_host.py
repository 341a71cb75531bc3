"""Gated weight-only fp8 GEMM1 without a GPU ("Gated weight-only GEMM1"): the C ABI declares and exports
``chipmunk_csp_mlp_mm1_glu_w8[_batched|_gm]`` and refuses bad arguments with a code and a message, before any launch; the wrapper raises
``ValueError``s that name the argument; the fake kernel gives shapes; the compiled code has exactly six ``mm1_glu_w8_kernel`` instantiations at
one tile shape, without VGPR spills, scratch or static LDS, under an LDS request of at most 80 KiB; the key ``mlp.w8_gated`` defaults to off
and switches what ``SparseDiffGatedMlp`` accepts; the error metric of tests/test_gpu_mlp_glu_w8.py is proven on the CPU: a torch stand-in of
the kernel's arithmetic lies inside ``MLP_SEG_BOUND`` of the fp64 model (tests/mlp_glu_w8_model.py), six mutants at least twice outside."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from helpers import MLP_BM, MLP_SEG_BOUND, MLP_SEG_W1, mlp_act64, mlp_group_cols, seg_rel_err
from mlp_glu_w8_model import mm1_glu_w8_exact
from mlp_w8_model import E4M3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = ("chipmunk_csp_mlp_mm1_glu_w8", "chipmunk_csp_mlp_mm1_glu_w8_batched", "chipmunk_csp_mlp_mm1_glu_w8_gm")


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_three_entries():
    from chipmunk_amd import _native
    header = open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read()
    for name in NAMES:
        assert name in _native.SYMBOLS and re.search(rf"\bint {name}\s*\(", header), name
        assert hasattr(_native.lib(), name), f"{name} is not exported"
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", header).group(1)
        assert re.search(r"const void \*b_gate,\s*const void \*b_up,\s*const float \*scale_gate,\s*int scale_gate_n,\s*const float \*scale_up,"
                         r"\s*int scale_up_n,", decl), f"{name}: the scales and their counts behind the two weights"
    assert _native.lib().chipmunk_abi_version() == 1


def _entries():
    """the three entries as call(**overrides) -> (code, message); no launch happens: every call below is refused"""
    from chipmunk_amd import _native
    lib, p, null = _native.lib(), ctypes.c_void_p(256), ctypes.c_void_p(0)
    i, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    head = [vp, vp, vp, vp, i, vp, i, vp, vp, vp, vp, vp, vp]
    lib.chipmunk_csp_mlp_mm1_glu_w8.argtypes = head + [i, i, i, i, i, i, vp]
    lib.chipmunk_csp_mlp_mm1_glu_w8_batched.argtypes = head + [i, i, i, i, i, i, i, i64, vp]
    lib.chipmunk_csp_mlp_mm1_glu_w8_gm.argtypes = head + [i, i, i, i, i, i, i64, vp]
    base = dict(a=p, bg=p, bu=p, sg=p, sgn=1, su=p, sun=1, c=p, biasg=null, biasu=null, cache=p, inds=p, cnt=p, M=100, K=128, F=256,
                ldc=104, act=0, upd=0)

    def head_of(v):
        return (v["a"], v["bg"], v["bu"], v["sg"], v["sgn"], v["su"], v["sun"], v["c"], v["biasg"], v["biasu"], v["cache"], v["inds"], v["cnt"])

    def single(**kw):
        v = dict(base, **kw)
        return lib.chipmunk_csp_mlp_mm1_glu_w8(*head_of(v), v["M"], v["K"], v["F"], v["ldc"], v["act"], v["upd"], null), _native.last_error()

    def batched(B=2, bs=256 * 104, **kw):
        v = dict(base, **kw)
        return (lib.chipmunk_csp_mlp_mm1_glu_w8_batched(*head_of(v), v["M"], v["K"], v["F"], v["ldc"], v["act"], v["upd"], B, bs, null),
                _native.last_error())

    def gm(B=1, bs=256 * 128, **kw):
        v = dict(base, **kw)
        return lib.chipmunk_csp_mlp_mm1_glu_w8_gm(*head_of(v), v["M"], v["K"], v["F"], v["act"], v["upd"], B, bs, null), _native.last_error()
    return single, batched, gm


NULL = ctypes.c_void_p(0)
REFUSALS = ((dict(a=NULL), "null"), (dict(bg=NULL), "null"), (dict(bu=NULL), "null"), (dict(sg=NULL), "null"), (dict(su=NULL), "null"),
            (dict(c=NULL), "null"), (dict(cache=NULL), "null"),
            (dict(sgn=0), "scale_gate_n must be 1"), (dict(sgn=2), "scale_gate_n must be 1"), (dict(sgn=128), "scale_gate_n must be 1"),
            (dict(sun=0), "scale_up_n must be 1"), (dict(sun=2), "scale_up_n must be 1"), (dict(sun=128), "scale_up_n must be 1"),
            (dict(sg=ctypes.c_void_p(258)), "4-byte aligned"), (dict(su=ctypes.c_void_p(257)), "4-byte aligned"),
            (dict(K=96), "multiple of 64"), (dict(K=0), "multiple of 64"),
            (dict(upd=2), "update_cache must be 0 or 1"), (dict(upd=-1), "update_cache must be 0 or 1"),
            (dict(act=3), "unknown activation"), (dict(act=-1), "unknown activation"),
            # ... and what check_mm1 refuses for the bf16 gated form
            (dict(inds=NULL), "indices / counts"), (dict(cnt=NULL), "indices / counts"),
            (dict(M=0), "M must be positive"), (dict(F=96), "multiple of 64"))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_every_entry_refuses_bad_arguments_before_any_launch(which):
    call = _entries()[which]
    for kw, text in REFUSALS:
        rc, msg = call(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)
    for kw in (dict(sgn=256), dict(sun=256), dict(sgn=256, sun=256)):    # _n == F passes that check: the next refusal is another one
        rc, msg = call(K=96, **kw)
        assert rc == 1 and "_n must be" not in msg and "multiple of 64" in msg, (kw, msg)


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


def test_wrapper_refusals_name_the_argument():
    """the wrapper's own checks, in front of the operator (no GPU: the operator's device check would come first for CPU tensors)"""
    from chipmunk_amd import ops
    from chipmunk_amd.ops.mlp import mm1_glu_w8, run_e2e_glu_w8
    assert ops.mlp_glu_w8 is run_e2e_glu_w8 and ops.mm1_glu_w8 is mm1_glu_w8 and "mlp_glu_w8" in ops.__all__
    bf16 = torch.bfloat16
    x, w8 = torch.zeros(128, 64, dtype=bf16), torch.zeros(64, 64).to(E4M3)
    packed, cache = torch.zeros(128, 64, dtype=bf16), torch.zeros(64, 128, dtype=bf16)
    inds, cnt, s = torch.zeros(1, 64, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.ones(())
    tail = (packed, None, None)
    with pytest.raises(ValueError, match="unknown activation"):
        mm1_glu_w8(x, w8, w8, s, s, *tail, "relu", cache, inds, cnt)
    with pytest.raises(ValueError, match="w_gate must be float8_e4m3fn"):
        mm1_glu_w8(x, w8.to(bf16), w8, s, s, *tail, "silu", cache, inds, cnt)
    with pytest.raises(ValueError, match="w_up must be float8_e4m3fn"):
        mm1_glu_w8(x, w8, w8.to(bf16), s, s, *tail, "silu", cache, inds, cnt)
    with pytest.raises(ValueError, match="x must be bfloat16"):
        mm1_glu_w8(x.to(E4M3), w8, w8, s, s, *tail, "silu", cache, inds, cnt)
    with pytest.raises(ValueError, match="scale_gate must hold one number"):
        mm1_glu_w8(x, w8, w8, torch.ones(3), s, *tail, "silu", cache, inds, cnt)
    with pytest.raises(ValueError, match="scale_up must hold one number"):
        mm1_glu_w8(x, w8, w8, s, torch.ones(64, 1), *tail, "silu", cache, inds, cnt)
    out = torch.zeros(128, 32, dtype=bf16)
    with pytest.raises(ValueError, match="scale_up must hold one number"):
        run_e2e_glu_w8(x, w8, w8, s, torch.ones(2), None, None, "silu", torch.zeros(64, 32, dtype=bf16), inds, cnt, cache, out, 0)


def test_fake_kernel_traces_without_a_gpu_and_checks_shapes():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        bf16 = torch.bfloat16
        a, c = torch.empty(2, 333, 128, dtype=bf16), torch.empty(2, 333, 512, dtype=bf16)
        fused = torch.empty(1024, 128, dtype=E4M3)
        wg, wu = fused[:512], fused[512:]
        cache, bias = torch.empty(2, 512, 333, dtype=bf16), torch.empty(512, dtype=bf16)
        inds, counts = torch.empty(2, 3, 512, dtype=torch.int32), torch.empty(2, 3, dtype=torch.int32)
        op = torch.ops.chipmunk.csp_mlp_mm1_glu_w8
        one, vec = torch.empty(1), torch.empty(512)
        for sg, su in ((one, one), (vec, one), (one, vec), (vec, vec)):
            assert op(a, wg, wu, sg, su, c, bias, None, cache, inds, counts, "silu", True) is None
            assert op(a[0], wu, wg, sg, su, c[0], None, bias, cache[0], inds[0], counts[0], "gelu", False) is None
        with pytest.raises(RuntimeError, match="float8_e4m3fn"):
            op(a, wg.to(bf16), wu, one, one, c, bias, None, cache, inds, counts, "silu", True)
        with pytest.raises(RuntimeError, match="one element, or \\[F\\]"):
            op(a, wg, wu, one, torch.empty(2), c, bias, None, cache, inds, counts, "silu", True)
        with pytest.raises(RuntimeError, match="c must be"):
            op(a, wg, wu, one, one, c[0], bias, None, cache, inds, counts, "silu", True)
        with pytest.raises(RuntimeError, match="unknown activation"):
            op(a, wg, wu, one, one, c, bias, None, cache, inds, counts, "relu", True)


# ------------------------------------------------------------------------------------------------------------------ compile audit
def test_six_kernels_at_one_tile_shape_without_spills_scratch_or_static_lds(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "mlp.s"        # (as tests/test_mlp_w8_host.py)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "chipmunk_amd", "csrc", "mlp.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    # mm1_glu_w8_kernel<BN, BK, NST, WPS, ACT, BATCHED>
    inst = re.compile(r"17mm1_glu_w8_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi([012])ELb([01])EEE")
    seen, shapes = set(), set()
    for block in text.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "mm1_glu_w8_kernel" not in name.group(1):
            continue
        m = inst.search(name.group(1))
        assert m, f"an unexpected gated weight-only GEMM1 instantiation: {name.group(1)}"
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spill == 0 and scratch == 0, f"{name.group(1)}: {spill} VGPR spills, {scratch} bytes of scratch"
        assert lds == 0, "the ring is dynamic LDS"
        assert (int(m.group(5)), int(m.group(6))) not in seen, f"{name.group(1)}: instantiated twice"
        shapes.add(tuple(int(v) for v in m.groups()[:4]))
        seen.add((int(m.group(5)), int(m.group(6))))
    assert seen == {(act, b) for act in (0, 1, 2) for b in (0, 1)}, f"mm1_glu_w8_kernel instantiations (act, batched): {sorted(seen)}"
    assert len(shapes) == 1, f"more than one tile shape: {sorted(shapes)}"
    bn, bk, nst, wps = next(iter(shapes))
    # the launcher's request: NST stages of 128 bf16 A rows and BN e4m3 B rows of one k step, + 16 bytes per 32 B rows (the shifted pieces)
    request = nst * (128 * bk * 2 + bn * bk + bn // 32 * 16)
    src = open(os.path.join(ROOT, "chipmunk_amd", "csrc", "mlp.hip")).read()
    launcher = src[src.index("int launch_mm1_glu_w8_kernel("):]
    launcher = launcher[: launcher.index("CM_LAUNCH_CHECK")]
    assert re.search(rf"constexpr int BN = {bn}, BK = {bk}, NST = {nst}, WPS = {wps};", launcher), "the launcher's shape is the kernels'"
    assert "constexpr int LDS = NST * (BM * BK * 2 + BN * BK + BN / 32 * 16);" in launcher and "static_assert(LDS <= 80 * 1024" in launcher
    assert "mm1_glu_w8_kernel<BN, BK, NST, WPS, ACT, BATCHED>" in launcher
    assert request <= 80 * 1024 and wps == 2, f"LDS request {request} bytes: two workgroups must share a CU"
    # the staged epilogue, not FLAT: the cache block and the output image (128 rows x BN / 2 packed columns, bf16) fit one stage each
    assert 128 * (bn // 2) * 2 <= request // nst


# ------------------------------------------------------------------------------------------------------------------ config, modules
def test_the_key_defaults_to_off_and_amd_key_serves_it(fresh_config):
    from chipmunk_amd.util import config as cfg
    assert cfg.AMD_EXTRA_KEYS["mlp.w8_gated"] is False and cfg.BASE_CONFIG["mlp"]["w8_gated"] is False
    assert cfg.amd_key("mlp", "w8_gated") is False
    fresh_config["mlp"]["w8_gated"] = True
    assert cfg.amd_key("mlp", "w8_gated") is True
    del fresh_config["mlp"]["w8_gated"]
    assert cfg.amd_key("mlp", "w8_gated") is False


def _makers():
    from chipmunk_amd.modules import SparseDiffGatedMlp, W8Linear
    from chipmunk_amd.util.layer_counter import LayerCounter
    plain = lambda i, o: torch.nn.Linear(i, o).bfloat16()      # noqa: E731
    w8 = lambda i, o, **kw: W8Linear.from_linear(plain(i, o), **kw)      # noqa: E731
    counter, silu = LayerCounter(1, 1), torch.nn.SiLU()
    two = lambda **kw: SparseDiffGatedMlp(0, counter, w8(128, 256, **kw), w8(128, 256, **kw), silu, plain(256, 128))      # noqa: E731
    mixed = lambda: SparseDiffGatedMlp(0, counter, w8(128, 256), plain(128, 256), silu, plain(256, 128))      # noqa: E731
    fused = lambda **kw: SparseDiffGatedMlp.from_fused(0, counter, w8(128, 512, **kw), silu, plain(256, 128))      # noqa: E731
    return two, mixed, fused


def test_key_off_refuses_and_key_on_accepts_all_but_the_mixed_pair(fresh_config):
    """construction only: no operator runs"""
    import chipmunk_amd  # noqa: F401
    two, mixed, fused = _makers()
    assert not fresh_config["mlp"]["w8_gated"]
    for make in (two, mixed, fused):
        with pytest.raises(ValueError, match="only the ungated GEMM1 has a weight-only form.*mlp.w8_gated"):
            make()
    fresh_config["mlp"]["w8_gated"] = True
    for scaling in ("tensor", "row"):
        m = two(scaling=scaling)
        assert m.w8 and not m.fp8 and m.gate[0].dtype == E4M3 and m.up[0].dtype == E4M3
        sg, su = m.w8_scales
        assert sg is m.projs[0].scale_reciprocal and su is m.projs[1].scale_reciprocal
        assert tuple(sg.shape) == ((256,) if scaling == "row" else ())
        f = fused(scaling=scaling)
        assert f.w8 and not f.fp8 and tuple(f.gate[0].shape) == (256, 128)
    with pytest.raises(ValueError, match="mixed pair"):
        mixed()
    # bf16 projections take the path they took
    from chipmunk_amd.modules import SparseDiffGatedMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    plain = lambda i, o: torch.nn.Linear(i, o).bfloat16()      # noqa: E731
    b = SparseDiffGatedMlp(0, LayerCounter(1, 1), plain(128, 256), plain(128, 256), torch.nn.SiLU(), plain(256, 128))
    assert not b.w8 and not b.fp8


@pytest.mark.parametrize("gate_first", [True, False])
def test_a_fused_scale_is_split_into_views_of_the_right_halves(fresh_config, gate_first):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd.modules import SparseDiffGatedMlp, W8Linear
    from chipmunk_amd.util.layer_counter import LayerCounter
    fresh_config["mlp"]["w8_gated"] = True
    torch.manual_seed(3)
    src = torch.nn.Linear(128, 512).bfloat16()
    with torch.no_grad():
        src.weight.mul_(torch.logspace(-2, 2, 512).unsqueeze(1).to(torch.bfloat16))
    fc1 = W8Linear.from_linear(src, scaling="row")
    m = SparseDiffGatedMlp.from_fused(0, LayerCounter(1, 1), fc1, torch.nn.SiLU(), torch.nn.Linear(256, 128).bfloat16(), gate_first=gate_first)
    (wg, bg), (wu, bu), (sg, su) = m.gate, m.up, m.w8_scales
    lo, hi = (slice(0, 256), slice(256, 512)) if gate_first else (slice(256, 512), slice(0, 256))
    s, w, b = fc1.scale_reciprocal, fc1.weight.data, fc1.bias.data
    for got, whole, rows in ((sg, s, lo), (su, s, hi), (wg, w, lo), (wu, w, hi), (bg, b, lo), (bu, b, hi)):
        part = whole[rows]
        assert got.data_ptr() == part.data_ptr() and got.shape == part.shape and got.stride() == part.stride(), "a view, not a copy"
        assert got.is_contiguous()
    assert not torch.equal(sg, su)
    # a [] scale serves both halves
    one = SparseDiffGatedMlp.from_fused(0, LayerCounter(1, 1), W8Linear.from_linear(src, scaling="tensor"), torch.nn.SiLU(),
                                        torch.nn.Linear(256, 128).bfloat16(), gate_first=gate_first)
    sg, su = one.w8_scales
    assert sg is su and sg.dim() == 0
    # the dense path calls the fused layer once and splits its output
    x = torch.randn(1, 5, 128).bfloat16()
    y = fc1(x)
    g, u = m._pre(x)
    assert torch.equal(g, y[..., lo]) and torch.equal(u, y[..., hi])


# ------------------------------------------------------------------------------------------------------------------ the error metric
ACTS = ("gelu_tanh", "silu", "gelu")
MUTANTS = ("scales swapped", "scale behind the bias", "up scale dropped", "scale read at the packed position", "weights swapped",
           "activation on the product")


def _metric_problem():
    """M = 200 (a ragged second group), K = 192, F = 256.  Pre-activations of order 0.4 (a 0.5, w 0.06, sqrt K = 13.9) with biases 0.3
    beside them; per-row scales no powers of two and spread over four octaves -- row i is quantised with (amax_i / 448) * 2^k_i, k_i in
    0 .. 3, which e4m3 (a floating-point format) represents as well as amax_i / 448 --, the up scales 1.7 times another draw."""
    g = torch.Generator().manual_seed(20)
    M, K, F = 200, 192, 256
    p = dict(M=M, K=K, F=F)
    p["a"] = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    for name, mul in (("g", 1.0), ("u", 1.7)):
        w = torch.randn(F, K, generator=g) * 0.06
        recip = (w.abs().amax(dim=1) / 448.0 * mul * torch.ldexp(torch.ones(F), torch.randint(0, 4, (F,), generator=g))).float()
        p["w" + name] = (w / recip[:, None]).to(E4M3)
        p["s" + name] = recip
        p["b" + name] = (torch.randn(F, generator=g) * 0.3).to(torch.bfloat16)
    p["cache"] = (torch.randn(F, M, generator=g) * 0.3).to(torch.bfloat16)
    p["inds"] = torch.stack([torch.randperm(F, generator=g) for _ in range(2)]).to(torch.int32)
    p["cnt"] = torch.tensor([256, 130], dtype=torch.int32)
    assert float(p["sg"].max() / p["sg"].min()) > 8 and not torch.equal(p["sg"], p["su"])
    return p


def _stand_in(p, act, mutant=None):
    """the kernel's arithmetic in torch: fp32 sums, sum * scale and + bias each rounded to fp32, act in fp32, fma(act(g), u, -cache) with
    one rounding to bf16 (the product of two fp32 numbers is exact in fp64) -> packed deltas [M, F] bf16"""
    M, F = p["M"], p["F"]
    out = torch.zeros(M, F, dtype=torch.bfloat16)
    wg, wu, sg, su = p["wg"], p["wu"], p["sg"], p["su"]
    if mutant == "scales swapped":
        sg, su = su, sg
    if mutant == "weights swapped":
        wg, wu = wu, wg
    if mutant == "up scale dropped":
        su = torch.ones_like(su)
    a = p["a"].float()
    for g in range(p["inds"].shape[0]):
        rows, n = slice(g * MLP_BM, min(M, (g + 1) * MLP_BM)), int(p["cnt"][g])
        col = p["inds"][g, :n].long()
        at = torch.arange(n) if mutant == "scale read at the packed position" else col
        sum_g, sum_u = a[rows] @ wg.float()[col].T, a[rows] @ wu.float()[col].T
        bg, bu = p["bg"][col].float(), p["bu"][col].float()
        if mutant == "scale behind the bias":
            hg, hu = (sum_g + bg) * sg[at], (sum_u + bu) * su[at]
        else:
            hg, hu = (sum_g * sg[at]) + bg, (sum_u * su[at]) + bu
        c = p["cache"][col][:, rows].T.double()
        if mutant == "activation on the product":
            d = mlp_act64(act, hg * hu).double() - c
        else:
            d = mlp_act64(act, hg).double() * hu.double() - c
        out[rows, :n] = d.to(torch.bfloat16)
    return out


@pytest.mark.parametrize("act", ACTS)
def test_the_stand_in_is_inside_the_bound_and_every_mutant_twice_outside(act):
    p = _metric_problem()
    exact, _ = mm1_glu_w8_exact(p["a"], p["wg"], p["wu"], p["sg"], p["su"], p["bg"], p["bu"], p["cache"], p["inds"], p["cnt"], act)
    cols = mlp_group_cols(p["cnt"], p["M"])
    worst = float(seg_rel_err(_stand_in(p, act), exact, MLP_SEG_W1, cols).max())
    print(f"{act}: stand-in worst 64-column segment error {worst:.5f} (bound {MLP_SEG_BOUND})")
    assert worst <= MLP_SEG_BOUND, f"{act}: the kernel's arithmetic lies {worst:.4g} from the fp64 model, outside {MLP_SEG_BOUND}"
    for mutant in MUTANTS:
        err = seg_rel_err(_stand_in(p, act, mutant), exact, MLP_SEG_W1, cols)
        got = float(err.max())
        print(f"{act}: mutant '{mutant}' worst segment error {got:.4g}, {float((err > MLP_SEG_BOUND).double().mean()):.2f} of the segments outside")
        assert got >= 2 * MLP_SEG_BOUND, f"{act}: mutant '{mutant}' at {got:.4g} is not twice outside the bound {MLP_SEG_BOUND}"
