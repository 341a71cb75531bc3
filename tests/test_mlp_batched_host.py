"""Batches (B > 1 sequences per launch) in the sparse MLP, the parts that need no GPU: the tile maps over B * G groups (a written-down model
of the kernels' arithmetic, tests/mlp_tile_model.py, tied to the source), the six *_batched entry points of the C ABI and their argument
checks, the resource use of the new kernel instantiations, and the module's stored state for a batch."""
import ctypes
import os
import re
import subprocess
from collections import Counter

import pytest
import torch

import mlp_tile_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chipmunk_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BATCHED = ["chipmunk_csp_mlp_mm1_batched", "chipmunk_csp_mlp_mm1_scatter_batched", "chipmunk_csp_mlp_mm1_fp8_batched",
           "chipmunk_csp_mlp_mm2_batched", "chipmunk_csp_mlp_mm2_and_scatter_add_batched", "chipmunk_csp_scatter_add_batched"]
P = ctypes.c_void_p(16)       # a non-null pointer: every call below fails its argument checks before anything is launched
NULL = ctypes.c_void_p(0)
I64 = ctypes.c_int64


# ------------------------------------------------------------------------------------------------ the tile maps
def _count_lists(B, G, F, seed):
    """B * G counts, different per sequence, each sequence's list holding a 0 and a full F where it has the room (multiples of 8)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in range(B):
        c = (torch.randint(0, F // 8 + 1, (G,), generator=g) * 8).tolist()
        c[b % G] = F
        if G > 1:
            c[(b + 1) % G] = 0
        out += c
    return out


# cus = 8 x resident-slots-per-XCD / 2: 256 is the MI355X; the small ones make the launches here multi-round, with and without a tail split
@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("M", [128, 1000, 1024, 333, 4352])
@pytest.mark.parametrize("F,cus", [(512, 256), (512, 8), (1536, 16), (1536, 24), (2048, 32)])
def test_gemm1_map_produces_every_live_unit_exactly_once(B, M, F, cus):
    G = (M + 127) // 128
    counts = _count_lists(B, G, F, seed=B * 1000 + M + F)
    got, _ = tm.gemm1_launch(counts, B, M, F, cus)
    want = tm.gemm1_live(counts, B, M)
    dup = [u for u, n in Counter(got).items() if n > 1]
    assert not dup, f"produced more than once: {dup[:5]}"
    assert set(got) == set(want), (sorted(set(want) - set(got))[:5], sorted(set(got) - set(want))[:5])
    # ... and without the split (option mm1_no_split) it is the same set
    assert sorted(tm.gemm1_launch(counts, B, M, F, cus, split=False)[0]) == sorted(want)


def test_gemm1_tail_split_is_taken_and_crosses_a_batch_boundary():
    """The shape of the GPU test: B = 2, M = 1000 (16 groups), slots / 2 + 1 live column tiles -> every XCD keeps two leftover tiles, handed
    out as sub-tiles, some of them in the second sequence."""
    cus = 256
    slots = 2 * cus // 8
    nt = slots // 2 + 1
    F = nt * 128
    B, M = 2, 1000
    counts = [2048, 0, 1024, 3072, 512, 256, 4096, F, 256, F, 0, 1024, 2048, 512, 3072, F]
    got, from_split = tm.gemm1_launch(counts, B, M, F, cus)
    assert sorted(got) == sorted(tm.gemm1_live(counts, B, M))
    pl = tm.plan_tiles(counts, 16, nt, 4, 0, 128, slots, 4)
    assert pl["mine"] == 2 * nt and pl["mine"] - pl["full"] == 2, pl
    assert from_split > 0
    nosplit, zero = tm.gemm1_launch(counts, B, M, F, cus, split=False)
    assert zero == 0 and sorted(nosplit) == sorted(got)
    # the sub-tiles of XCD 7 end the launch's tile list: the last tiles of the LAST group, which belongs to sequence 1
    pl7 = tm.plan_tiles(counts, 16, nt, 4, 7, 128, slots, 4)
    seqs = {tm.sequence_of(tm.tile_at(pl7, s)[0], 8)[0] for s in range(pl7["full"], pl7["slots"])}
    assert 1 in seqs


@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("M", [128, 1000, 1024, 333, 4352])
@pytest.mark.parametrize("N2,cus", [(256, 256), (1536, 256), (3072, 256), (3072, 32), (264, 8)])
def test_gemm2_map_produces_every_tile_exactly_once(B, M, N2, cus):
    G = (M + 127) // 128
    counts = _count_lists(B, G, 512, seed=B + M + N2)
    want = tm.gemm2_live(counts, B, M, N2)
    for order in (True, False):
        got = tm.gemm2_launch(counts, B, M, N2, cus, order=order)
        assert len(got) == len(set(got)) and sorted(got) == sorted(want), (B, M, N2, cus, order)


def test_groups_map_to_sequences():
    assert [tm.sequence_of(g, 3) for g in range(7)] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0)]


def test_model_constants_are_the_kernels():
    src = open(os.path.join(CSRC, "mlp.hip")).read()
    assert re.search(r"constexpr int BM = (\d+);", src).group(1) == str(tm.BM)
    assert "const int xcd = blockIdx.x & 7;" in src and tm.XCDS == 8
    assert "constexpr int NSUB = NW == 4 ? 2 * (BN / 64) : 1;" in src and tm.nsub(128) == 4
    assert f"return launch_mm1_variant<{tm.GEMM1_BN}, 64, 2, {tm.GEMM1_WPS}>(p, stream, cache_updated);" in src
    assert f"return launch_mm1_variant<{tm.GEMM1_BN}, 64, 2, {tm.GEMM1_WPS}, false, 4, true>(p, stream, cache_updated, B, cache_bs);" in src
    assert f"return launch_mm1_variant<{tm.GEMM1_BN}, 64, 2, {tm.GEMM1_WPS}, true, 4, true>(p, stream, nullptr, B, cache_bs);" in src
    assert f"return launch_mm2_variant<{tm.GEMM2_BN}, 32, 3, 2, 8>(p, s);" in src
    assert f"return launch_mm2_variant<{tm.GEMM2_BN}, 32, 3, 2, 8, true>(p, s, B);" in src
    assert len(re.findall(r'chipmunk_get_option\("mm[12]_nr"\) : (\d+);', src)) == 2
    assert set(re.findall(r'chipmunk_get_option\("mm[12]_nr"\) : (\d+);', src)) == {str(tm.NR)}
    # the walk the model writes out: sequence = group / groups-per-sequence, in all three kernels
    assert src.count("const int b = tm.g / Gs;") == src.count(" g = tm.g - b * Gs;") == 2      # (mm1_kernel, mm1_form_kernel)
    assert "bseq = gi / Gs;" in src and "b = blockIdx.y / Gs;" in src


# ------------------------------------------------------------------------------------------------ the C ABI
def test_batched_entry_points_are_declared_exported_and_listed():
    from chipmunk_amd import _native
    text = open(os.path.join(ROOT, "include", "chipmunk_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _native.lib()
    for name in BATCHED:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/chipmunk_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SYMBOLS
    assert lib.chipmunk_abi_version() == 1


def _calls(M=333, ldc=336, B=2, bs=512 * 336, ptr=P, idx=P):
    """name -> call of every batched entry point, K = 256, F = 512, N2 = 256"""
    from chipmunk_amd import _native
    lib = _native.lib()
    bs = I64(bs)
    return {
        "mm1": lambda: lib.chipmunk_csp_mlp_mm1_batched(ptr, P, P, P, P, idx, P, M, 256, 512, ldc, B, bs, NULL),
        "mm1_scatter": lambda: lib.chipmunk_csp_mlp_mm1_scatter_batched(ptr, P, P, P, P, idx, P, M, 256, 512, ldc, B, bs, NULL),
        "mm1_fp8": lambda: lib.chipmunk_csp_mlp_mm1_fp8_batched(ptr, P, P, P, P, idx, P, P, P, M, 256, 512, ldc, 0, B, bs, NULL),
        "mm2": lambda: lib.chipmunk_csp_mlp_mm2_batched(ptr, P, P, idx, P, M, 512, 256, B, NULL),
        "mm2_and_scatter_add": lambda: lib.chipmunk_csp_mlp_mm2_and_scatter_add_batched(ptr, P, idx, P, P, P, P, M, 512, 256, ldc, B, bs, NULL),
        "scatter_add": lambda: lib.chipmunk_csp_scatter_add_batched(ptr, P, idx, P, M, 512, ldc, B, bs, NULL),
    }


def test_null_pointers_return_a_code():
    from chipmunk_amd import _native
    for name, call in _calls(ptr=NULL).items():
        assert call() == 1 and "null" in _native.last_error(), (name, _native.last_error())
    for name, call in _calls(idx=NULL).items():
        assert call() == 1 and "indices" in _native.last_error(), (name, _native.last_error())


@pytest.mark.parametrize("B", [0, -1])
def test_batch_size_below_one_is_refused(B):
    from chipmunk_amd import _native
    for name, call in _calls(B=B).items():
        assert call() == 1, name
        assert "batch size B must be at least 1" in _native.last_error(), (name, _native.last_error())


@pytest.mark.parametrize("M,ldc", [(333, 328), (333, 333), (333, 340), (129, 0)])
def test_bad_pitch_returns_a_code_and_names_the_rule(M, ldc):
    from chipmunk_amd import _native
    for name, call in _calls(M=M, ldc=ldc, bs=512 * 1024).items():
        if name == "mm2":
            continue      # takes no cache
        assert call() == 1, name
        msg = _native.last_error()
        assert "ldc" in msg and "multiple of 8" in msg and "at least M" in msg, (name, msg)


@pytest.mark.parametrize("bs", [512 * 336 - 8, 512 * 336 + 4, 0, -8])
def test_bad_batch_stride_returns_a_code_and_names_the_rule(bs):
    from chipmunk_amd import _native
    for name, call in _calls(bs=bs).items():
        if name == "mm2":
            continue
        assert call() == 1, name
        msg = _native.last_error()
        assert "batch stride" in msg and "F * ldc" in msg and "multiple of 8" in msg, (name, msg)


def test_too_many_groups_returns_a_code_and_names_the_rule():
    from chipmunk_amd import _native
    # 3 groups per sequence: 21 845 sequences are 65 535 groups, one more is too many
    for name, call in _calls(B=21846).items():
        assert call() == 1, name
        assert "65535" in _native.last_error() and "groups" in _native.last_error(), (name, _native.last_error())
    # at the limit the next check is the one that fails (K must be a multiple of 64 / N2 of 8), not the group count
    lib = _native.lib()
    assert lib.chipmunk_csp_mlp_mm1_batched(P, P, P, P, P, P, P, 333, 100, 512, 336, 21845, I64(512 * 336), NULL) == 1
    assert "K must be" in _native.last_error()
    assert lib.chipmunk_csp_mlp_mm2_batched(P, P, P, P, P, 333, 512, 100, 21845, NULL) == 1 and "N2 must be" in _native.last_error()


def test_the_existing_entries_keep_their_checks():
    from chipmunk_amd import _native
    lib = _native.lib()
    assert lib.chipmunk_csp_mlp_mm1(P, P, P, P, P, P, P, 100, 64, 256, NULL) == 1 and "multiple of 128" in _native.last_error()
    assert lib.chipmunk_csp_scatter_add(P, P, P, P, 1000, 512, 6, NULL) == 1 and "multiple of 128" in _native.last_error()
    assert lib.chipmunk_csp_mlp_mm2(P, P, P, P, P, 1000, 512, 256, NULL) == 1 and "multiple of 128" in _native.last_error()
    assert lib.chipmunk_csp_mlp_mm1_ragged(P, P, P, P, P, P, P, 333, 256, 512, 333, NULL) == 1 and "ldc" in _native.last_error()
    assert lib.chipmunk_csp_mlp_mm1_ragged(P, P, P, P, P, P, P, 100, 100, 256, 104, NULL) == 1 and "K must be" in _native.last_error()
    assert lib.chipmunk_csp_scatter_add_ragged(NULL, P, P, P, 333, 512, 336, NULL) == 1 and "null" in _native.last_error()


# ------------------------------------------------------------------------------------------------ the compiled kernels
def test_batched_kernel_instantiations_use_no_scratch(tmp_path):
    """GEMM1 bf16 and fp8, GEMM2 and scatter-add over B * G groups: each is an instantiation of its own beside the single-sequence one, and
    each compiles for gfx950 without spills and without scratch memory."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "mlp.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(CSRC, "mlp.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    names = re.findall(r"\.name:\s+(\S+)", text)
    scratch = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert len(names) == len(scratch) == len(spills)
    demangled = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    seen = set()
    for kname, sc, sp in zip(demangled, scratch, spills):
        assert int(sp) == 0 and int(sc) == 0, f"{kname}: {sp} spills, {sc} bytes of scratch"
        m = re.search(r"(mm1_kernel<128, 64, 2, 2, (?:false|true), 4, true>|mm2_kernel<256, 32, 3, 2, 8, true>|scatter_add_kernel<long>)", kname)
        if m:
            seen.add(m.group(1))
    assert len(seen) == 4, (seen, demangled)
    # ... beside the single-sequence instantiations, which stay
    for single in ("mm1_kernel<128, 64, 2, 2, false, 4, false>", "mm1_kernel<128, 64, 2, 2, true, 4, false>", "mm2_kernel<256, 32, 3, 2, 8, false>",
                   "scatter_add_kernel<>"):
        assert any(single in d for d in demangled), (single, demangled)


# ------------------------------------------------------------------------------------------------ the module
def test_module_on_cpu_stores_a_batch(fresh_config):
    """A full step of SparseDiffMlp at B = 2, N = 203 (plain torch on the CPU) stores the activation cache [2, F, 208] with zeroed padding,
    the output cache [2, 203, C] and the block means [2, 2, F]."""
    from chipmunk_amd.modules import SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    cfg = fresh_config
    cfg["offloading"]["global_disable_offloading"] = True
    cfg["mlp"].update(dict(top_keys=0.3, random_keys=0.0, full_step_every=4, first_n_dense_layers=0))
    torch.manual_seed(0)
    B, N, K, F = 2, 203, 16, 64
    fc1, fc2 = torch.nn.Linear(K, F), torch.nn.Linear(F, K)
    act = torch.nn.GELU(approximate="tanh")
    mlp = SparseDiffMlp(0, LayerCounter(1, 1), fc1, act, fc2, 6)
    x = torch.randn(B, N, K)
    with torch.no_grad():
        out = mlp(x)
        a = act(fc1(x))
    stored = mlp.storage.get_sparse_act_T()
    assert stored.shape == (B, F, 208) and stored.is_contiguous()
    assert torch.equal(stored[..., :N], a.transpose(1, 2)) and (stored[..., N:] == 0).all()
    assert mlp.storage.get_out_cache().shape == (B, N, K) and out.shape == (B, N, K)
    assert mlp.storage.get_blockmean_mid_cache().shape == (B, 2, F)
    assert not torch.equal(stored[0], stored[1])


def test_module_refuses_a_sparse_step_at_another_batch_size(fresh_config):
    from chipmunk_amd.modules import SparseDiffMlp
    from chipmunk_amd.util.layer_counter import LayerCounter
    cfg = fresh_config
    cfg["offloading"]["global_disable_offloading"] = True
    cfg["mlp"].update(dict(top_keys=0.3, random_keys=0.0, full_step_every=4, first_n_dense_layers=0))
    torch.manual_seed(0)
    fc1, fc2 = torch.nn.Linear(16, 64), torch.nn.Linear(64, 16)
    mlp = SparseDiffMlp(0, LayerCounter(1, 1), fc1, torch.nn.GELU(approximate="tanh"), fc2, 6)
    with torch.no_grad():
        mlp(torch.randn(2, 203, 16))
        with pytest.raises(RuntimeError, match="batch size 2 with 203 tokens"):
            mlp(torch.randn(3, 203, 16))
