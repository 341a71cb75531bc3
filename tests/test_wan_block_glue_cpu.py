"""Wan's block glue without a GPU: the CPU path of ``ops.residual_ln_modulate_f32`` (the reference's torch sequence,
``examples/wan/wan/modules/model.py:100-110, 317-334``) against the fp64 definition of tests/wan_block_glue_model.py over every input
family -- the floors, pinned tight --, ``x_out`` bit for bit against torch's fp32 formula, the mutants that ``MARGIN * floor`` must reject
(counted: at twice the bound or more wherever they apply, bit-inert where they cannot; recorded: printed), the fake kernel under a
full-graph trace, every refusal through the wrapper and through ctypes, and the compiled kernel's resources from the code object's
metadata.  docs/TEST_SENSITIVITY.md, "Wan block glue", has the tables this file prints (``pytest -s -k table``)."""
import ctypes
import functools
import os
import re
import subprocess

import pytest
import torch

import wan_block_glue_model as gm
from helpers import assert_rowwise_close, seg_rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chipmunk_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
XDTYPES = (torch.float32, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ cases (CPU sizes)
def _cases(mutants=False):
    """name -> arguments.  Floors: the shapes of tests/test_gpu_wan_block_glue.py.  mutants: three widths, a batch of two and of three."""
    out = {}
    shapes = [(2, 35, 8), (3, 24, 520), (2, 35, 1536)] if mutants else [(gm.BATCH, gm.SEQ_LEN, c) for c in gm.COLS]
    for B, L, C in shapes:
        for xdtype in XDTYPES:
            for residual in gm.RESIDUALS:
                if gm.refused(xdtype, residual):
                    continue
                for mod in gm.MODS:
                    for fam in gm.ALL:
                        name = f"B{B} L{L} C{C} {'fp32' if xdtype == torch.float32 else 'bf16'} {residual} {mod} {fam}"
                        out[name] = dict(B=B, L=L, C=C, xdtype=xdtype, residual=residual, mod=mod, family=fam, seed=7000 + len(out))
    return out


def _run(c, defects=()):
    """One case: the CPU path against the exact reference -- the worst full segment, the worst few-element segment as a share of its bound
    -- and per defect (worst error / bound, inert)."""
    from chipmunk_amd.ops import residual_ln_modulate_f32
    t = gm.glue_inputs(c["family"], c["B"], c["L"], c["C"], c["xdtype"], c["residual"], c["mod"], c["seed"])
    x, y, gate = t["x"], t["y"], t["gate"]
    rx, rxm = residual_ln_modulate_f32(**t, eps=gm.EPS)
    assert rxm.dtype == torch.bfloat16 and rxm.shape == x.shape
    if y is None:
        assert rx is x
    else:                                                            # a condition, not a tolerance
        assert rx.dtype == torch.float32 and torch.equal(rx.view(torch.int32), gm.residual_f32(x, y, gate).view(torch.int32)), "x_out"
    affine = t["weight"] is not None
    cls = gm.rounding_class(x, y, affine)
    args = (x, y, gate, t["shift"], t["scale"], t["weight"], t["bias"])
    exact, prod = gm.glue_exact(*args, x_out=rx if y is not None else None, with_prod=True)
    bound, few = gm.bound(cls, exact, prod)
    err = seg_rel_err(rxm, exact, gm.SEG_W)
    res = {"cls": cls, "floor": float(err[~few].max()) if (~few).any() else None, "few": float((err / bound)[few].max()) if few.any() else None,
           "mut": {}}
    assert_rowwise_close(rxm, exact, bound, "CPU path", width=gm.SEG_W)
    if defects:
        base = gm.glue_exact(*args, rounded=True, defect=gm.NO_DEFECT)
        same = lambda a, b: torch.equal(a.nan_to_num(nan=1e300), b.nan_to_num(nan=1e300))      # noqa: E731
        for d in defects:
            m = gm.glue_exact(*args, rounded=True, defect=d)
            ratio = float((seg_rel_err(m, exact, gm.SEG_W) / bound).max())
            res["mut"][d] = (ratio, same(m, base), gm.applies(d, t), gm.counted(d, t, c["family"]))
    return res


@functools.lru_cache(maxsize=None)
def _floors():
    """(class, family) -> (smallest, largest) worst full segment over the cases; and the worst few-element share"""
    table, few = {}, 0.0
    for name, c in _cases().items():
        r = _run(c)
        if r["floor"] is not None:
            lo, hi = table.get((r["cls"], c["family"]), (r["floor"], r["floor"]))
            table[(r["cls"], c["family"])] = (min(lo, r["floor"]), max(hi, r["floor"]))
        if r["few"] is not None:
            few = max(few, r["few"])
    return table, few


@functools.lru_cache(maxsize=None)
def _mutants():
    return {name: (c, _run(c, gm.DEFECTS + gm.RECORDED + (gm.NO_DEFECT,))["mut"]) for name, c in _cases(mutants=True).items()}


# ------------------------------------------------------------------------------------------------ the model's own arithmetic
def test_exact_reference_is_the_definition():
    t = gm.glue_inputs("iid", 2, 3, 24, torch.float32, "gated", "seq", 5)
    x, y, g, sh, sc = t["x"], t["y"], t["gate"], t["shift"], t["scale"]
    assert g.shape == (2, 1, 24) and sh.shape == sc.shape == (2, 24) and not torch.equal(sh[0], sh[1]) and not torch.equal(g[0], g[1])
    xm = gm.glue_exact(x, y, g, sh, sc, None, None)
    for b in range(2):
        for r in range(3):
            row = (x[b, r] + y[b, r].float() * g[b, 0]).double()      # fp32 product, fp32 sum
            want = (row - row.mean()) / (row.var(unbiased=False) + gm.EPS).sqrt() * (1 + sc[b].double()) + sh[b].double()
            assert torch.allclose(xm[b, r], want, rtol=1e-13, atol=1e-15)
    t = gm.glue_inputs("iid", 2, 3, 24, torch.bfloat16, "none", "affine", 6)
    xm = gm.glue_exact(t["x"], None, None, None, None, t["weight"], t["bias"])
    row = t["x"][1, 2].double()
    assert torch.allclose(xm[1, 2], (row - row.mean()) / (row.var(unbiased=False) + gm.EPS).sqrt() * t["weight"].double() + t["bias"].double(), rtol=1e-13)
    assert gm.rounding_class(t["x"], None, True) == "one" and gm.rounding_class(t["x"], None, False) == "two"
    assert gm.rounding_class(t["x"], t["x"], False) == "one" and gm.rounding_class(t["x"].float(), None, False) == "one"


def test_input_families_contain_what_they_promise():
    t = gm.glue_inputs("special", 2, 35, 520, torch.float32, "gated", "seq", 0)
    x, y = t["x"].reshape(70, 520).double(), t["y"].reshape(70, 520)
    assert not x[5].any() and not x[69].any() and (x[8] == 3.0).all() and abs(float(x[9].mean()) - 100) < 1 and 3 < float(x[9].std()) < 5
    assert abs(float(x[6].var(unbiased=False)) / gm.EPS - 1) < 0.02 and x[6, 0] != 0 and x[7, 519] != 0 and not x[7, :519].any()
    assert not y[5].any() and not y[8].any() and y[9].any()          # the mean-100 row keeps its y
    lad = gm.glue_inputs("ladder", 2, 35, 520, torch.float32, "none", "vec", 1)["x"].reshape(70, 520).double().var(-1, unbiased=False)
    assert float(lad.min()) < gm.EPS / 2 and float(lad.max()) > 1e4
    v = gm.glue_inputs("iid", 2, 35, 520, torch.bfloat16, "gated", "vec", 2)
    assert v["gate"].shape == v["shift"].shape == (520,) and v["x"].dtype == torch.bfloat16 and v["gate"].dtype == torch.float32
    assert 0.5 < float(v["gate"].std()) < 2 and 0.5 < float(v["shift"].std()) < 2          # of order 1


# ------------------------------------------------------------------------------------------------ floors
def test_cpu_path_is_under_its_floor_and_x_out_is_torchs_fp32_sum():
    """(`_run` also asserts, per case: x_out bit-equal to ``x.float() + y.float() * gate``, the caller's x handed back without y, every
    segment -- the few-element ones with their worst-case bound -- under its bound)"""
    table, few = _floors()
    for (cls, fam), (_, hi) in table.items():
        assert hi <= gm.FLOOR[cls], (cls, fam, hi)
    assert few <= 1.0


def test_floor_constants_are_tight():
    """every pinned constant is the measured maximum over families and cases rounded up, not a generous guess"""
    worst = {}
    for (cls, _), (_, hi) in _floors()[0].items():
        worst[cls] = max(worst.get(cls, 0.0), hi)
    assert set(worst) == set(gm.FLOOR)
    for cls, w in worst.items():
        assert w <= gm.FLOOR[cls] <= w + 1e-4, (cls, w)


def test_floor_table():
    table, few = _floors()
    print("\nclass | " + " | ".join(gm.ALL))
    for cls in sorted(gm.FLOOR):
        cells = [("" if (cls, f) not in table else f"{table[(cls, f)][0]:.4f} .. {table[(cls, f)][1]:.4f}") for f in gm.ALL]
        print(f"{cls} | " + " | ".join(cells) + f" | pinned {gm.FLOOR[cls]}")
    print(f"few-element segments: worst {few:.3f} of their bound")


# ------------------------------------------------------------------------------------------------ mutants
def test_every_counted_mutant_is_rejected_and_inert_where_it_cannot_apply():
    seen = {}
    for name, (c, muts) in _mutants().items():
        for d in gm.DEFECTS:
            ratio, inert, applies, counted = muts[d]
            if not applies:
                assert inert, f"{name}: '{d}' was expected to touch nothing"
            elif counted:
                assert not inert, f"{name}: '{d}' touches nothing"
                assert ratio >= 2.0, f"{name}: mutant '{d}' is at {ratio:.3f} of the bound, under twice it"
                seen[(d, c["family"])] = seen.get((d, c["family"]), 0) + 1
        assert muts[gm.NO_DEFECT][0] <= 1.0, (name, muts[gm.NO_DEFECT])      # the exact result rounded where the operator rounds
    for d in gm.DEFECTS:
        for fam in gm.FAMILIES[d]:
            assert seen.get((d, fam), 0) >= 2, (d, fam)


def test_mutant_table():
    """prints the table of docs/TEST_SENSITIVITY.md: per defect and family the weakest .. strongest case, error / bound"""
    table = {}
    for name, (c, muts) in _mutants().items():
        for d, (ratio, inert, applies, counted) in muts.items():
            if applies and not inert and (counted or c["family"] not in gm.FAMILIES.get(d, ())):      # (a counted family: its counted cases)
                lo, hi, n = table.setdefault(d, {}).get(c["family"], (ratio, ratio, 0))
                table[d][c["family"]] = (min(lo, ratio), max(hi, ratio), n + 1)
    print("\nmutant | " + " | ".join(f"{f}: error / bound, weakest .. strongest case" for f in gm.ALL))
    weakest = (float("inf"), None)
    for d in gm.DEFECTS + gm.RECORDED:
        cells = []
        for f in gm.ALL:
            t = table.get(d, {}).get(f)
            counted = d in gm.DEFECTS and f in gm.FAMILIES[d]
            cells.append("" if t is None else f"{'' if counted else '('}{t[0]:.3g} .. {t[1]:.3g}{'' if counted else ')'}")
            if t is not None and counted:
                weakest = min(weakest, (t[0], (d, f)))
        print(f"{'' if d in gm.DEFECTS else 'recorded: '}{d} | " + " | ".join(cells))
    print(f"weakest counted: {weakest}")
    assert weakest[0] >= 2.0, weakest
    # the stand-in is no substitute: on the mean-100 rows the bf16 stream alone is far outside the bound
    assert table[gm.BF16_POINTS]["special"][0] >= 2.0


# ------------------------------------------------------------------------------------------------ wrapper: shapes and refusals
def test_vector_shapes_are_one_operator():
    from chipmunk_amd.ops import residual_ln_modulate_f32
    t = gm.glue_inputs("iid", 2, 5, 24, torch.float32, "gated", "seq", 11)
    a = residual_ln_modulate_f32(**t)
    u = dict(t, gate=t["gate"].reshape(2, 24), shift=t["shift"].reshape(2, 1, 24), scale=t["scale"].reshape(2, 1, 24))
    b = residual_ln_modulate_f32(**u)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for s in range(2):                                              # a 2-D x is one sequence; a batch is its sequences
        one = residual_ln_modulate_f32(t["x"][s], t["y"][s], t["gate"][s, 0], t["shift"][s], t["scale"][s])
        assert one[0].shape == (5, 24) and torch.equal(one[0], a[0][s]) and torch.equal(one[1], a[1][s])


def test_argument_errors_of_the_python_wrapper():
    from chipmunk_amd.ops import residual_ln_modulate_f32 as f
    x, y = torch.zeros(2, 4, 16), torch.zeros(2, 4, 16, dtype=torch.bfloat16)
    v, w = torch.zeros(16), torch.ones(16)
    f(x, y, v, v, v)                                                                    # (the accepted form)
    bad = [
        dict(x=x, gate=v, shift=v, scale=v),                                            # a gate without y
        dict(x=x.bfloat16(), y=y, shift=v, scale=v),                                    # bf16 x with an ungated residual
        dict(x=x, y=y, gate=v),                                                         # neither modulation nor affine
        dict(x=x, shift=v, scale=v, weight=w, bias=v),                                  # both
        dict(x=x, shift=v), dict(x=x, weight=w),                                        # half a pair
        dict(x=torch.zeros(2, 4, 12), shift=torch.zeros(12), scale=torch.zeros(12)),    # C % 8
        dict(x=torch.zeros(1, 2, 8200), shift=torch.zeros(8200), scale=torch.zeros(8200)),      # C > 8192
        dict(x=x, shift=torch.zeros(3, 16), scale=torch.zeros(3, 16)),                  # a batch dimension that is neither 1 nor B
        dict(x=x, y=y, gate=torch.zeros(3, 1, 16), shift=v, scale=v),
        dict(x=x, shift=v.bfloat16(), scale=v.bfloat16()),                              # a modulation that is not fp32
        dict(x=x, y=y, gate=v.double(), shift=v, scale=v),
        dict(x=x, y=y.float(), gate=v, shift=v, scale=v),                               # y must be bf16
        dict(x=x, weight=torch.ones(2, 16), bias=torch.zeros(2, 16)),                   # the affine pair has no batch dimension
        dict(x=x.double(), shift=v, scale=v),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            f(**kw)


# ------------------------------------------------------------------------------------------------ fake kernel
def test_fake_kernel_shapes_and_full_graph_trace():
    import chipmunk_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.chipmunk.residual_ln_modulate_f32
    with FakeTensorMode():
        x, y, e = torch.empty(2, 100, 1536), torch.empty(2, 100, 1536, dtype=torch.bfloat16), torch.empty(2, 1536)
        xo, xm = op(x, y, e, e, e, None, None, 1e-6)
        assert xo.shape == xm.shape == (2, 100, 1536) and xo.dtype == torch.float32 and xm.dtype == torch.bfloat16 and xm.is_contiguous()
        xo, xm = op(x.bfloat16(), y, e, None, None, e[0], e[0], 1e-6)
        assert xo.dtype == torch.float32 and xm.dtype == torch.bfloat16                 # block 0: the stream becomes fp32
        (xm,) = op(x.bfloat16(), None, None, e, e, None, None, 1e-6)
        assert xm.dtype == torch.bfloat16 and xm.shape == x.shape

    def step(x, y, e, w):
        x, xm = op(x, y, e, e, e, None, None, 1e-6)
        (x3,) = op(x, None, None, None, None, w, w, 1e-6)
        return x, xm.float() + x3.float()

    with FakeTensorMode(allow_non_fake_inputs=True):                                    # (no kernel runs: fake inputs all the way)
        x, y, e = torch.empty(2, 100, 1536), torch.empty(2, 100, 1536, dtype=torch.bfloat16), torch.empty(2, 1, 1536)
        a, b = torch.compile(step, backend="eager", fullgraph=True)(x, y, e, torch.empty(1536))
        assert a.shape == b.shape == (2, 100, 1536) and a.dtype == b.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ C ABI
def _call(lib, *, x=4096, xd=2, y=8192, gate=12288, gs=0, shift=16384, scale=20480, ms=0, weight=0, bias=0, x_out=24576, xm=28672, B=2, L=16,
          cols=512):
    p = ctypes.c_void_p
    return lib.chipmunk_residual_ln_modulate_f32(p(x), ctypes.c_int(xd), p(y), p(gate), ctypes.c_int64(gs), p(shift), p(scale), ctypes.c_int64(ms),
                                                 p(weight), p(bias), p(x_out), p(xm), ctypes.c_int64(B), ctypes.c_int64(L), ctypes.c_int(cols),
                                                 ctypes.c_double(1e-6), p(0))


def test_c_entry_point_is_exported_and_refuses_bad_arguments_before_touching_a_gpu():
    """Every refusal returns CHIPMUNK_ERR_INVALID (1) with a message that names the rule; the pointers are made-up addresses, so a check
    that ran after a launch would not return at all.  (The C entry takes float pointers: a modulation that is not fp32 is a refusal of the
    layers above it.)"""
    from chipmunk_amd import _native
    lib = _native.lib()
    assert hasattr(lib, "chipmunk_residual_ln_modulate_f32") and "chipmunk_residual_ln_modulate_f32" in _native.SYMBOLS
    cases = [
        (dict(y=0, x_out=0), "a gate without y"),
        (dict(xd=1, gate=0), "with a gate"),
        (dict(shift=0, scale=0), "exactly one of"),
        (dict(weight=4096, bias=4096), "exactly one of"),
        (dict(scale=0), "come together"),
        (dict(shift=0, scale=0, weight=4096), "come together"),
        (dict(cols=516), "multiple of 8"),
        (dict(cols=8200), "at most 8192"),
        (dict(gs=8), "batch stride"),                                 # a stride that does not cover the row: a batch dimension that is not B
        (dict(ms=514), "batch stride"),
        (dict(shift=0, scale=0, weight=4096, bias=8192, ms=512), "batch stride"),
        (dict(gate=0, gs=512), "batch stride"),
        (dict(xd=3), "dtype code"),
        (dict(x_out=0), "come together"),
        (dict(y=0), "come together"),
        (dict(x=4096 + 8), "16-byte aligned"),
        (dict(shift=16384 + 4), "16-byte aligned"),
        (dict(B=0), "B must be"),
        (dict(x=0), "null pointer"),
    ]
    for kw, msg in cases:
        assert _call(lib, **kw) == 1, kw
        assert msg in _native.last_error(), (kw, _native.last_error())
    assert _call(lib, L=0) == 0                                       # nothing to do is not an error


# ------------------------------------------------------------------------------------------------ compile audit
def test_every_instantiation_compiles_without_spills_scratch_or_lds_and_with_16_byte_accesses(tmp_path):
    """As tests/test_wan_glue_host.py: compile rowwise.hip to gfx950 assembly (no GPU needed) and read each
    residual_ln_modulate_f32_kernel instantiation's metadata and body: the launcher's five row-length classes x {fp32, bf16} x x {with,
    without} y."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "rowwise.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(CSRC, "rowwise.hip"),
                           "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    docs = [d for d in re.split(r"\n  - (?=\.)", text[text.index("amdhsa.kernels:"):]) if ".name:" in d]   # one entry per kernel
    seen = set()
    for d in docs:
        name = re.search(r"\.name:\s+(\S+)", d).group(1)
        if "residual_ln_modulate_f32_kernel" not in name:
            continue
        field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", d).group(1))   # noqa: E731
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0 and field("agpr_count") == 0, name
        assert field("private_segment_fixed_size") == 0, f"{name}: scratch"
        assert field("group_segment_fixed_size") == 0, f"{name}: LDS"
        assert not re.search(r"\.uses_dynamic_stack:\s+true", d), name
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, name
        assert not re.search(r"\b(scratch_|ds_read|ds_write|ds_load|ds_store|buffer_store|v_accvgpr)", body), name
        narrow = re.findall(r"\bglobal_(?:load|store)_(?:dword|dwordx2|dwordx3|short|ushort|ubyte|byte|sbyte|sshort)\b", body)
        assert not narrow, f"{name}: global accesses narrower than 16 bytes: {sorted(set(narrow))}"
        nv, xbf, res = re.search(r"kernelILi(\d+)ELb([01])ELb([01])E", name).groups()
        seen.add((int(nv), int(xbf), int(res)))
    assert seen == {(nv, xbf, res) for nv in (2, 3, 6, 10, 16) for xbf in (0, 1) for res in (0, 1)}, seen
