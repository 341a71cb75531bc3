"""Host checks for the length-independent top-k mask: the written-down rule (tests/topk_mask_model.py) against torch.topk where
torch.topk is defined, the compiled streaming kernel's resource use, and the one ceiling the layers share."""
import os
import re
import subprocess

import pytest
import torch

from topk_mask_model import bf16_keys, topk_mask_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chipmunk_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _distinct_bf16_rows(rows, n, seed):
    """rows x n bf16 values, all distinct within a row (positive normal bf16 bit patterns, permuted): no ties."""
    g = torch.Generator().manual_seed(seed)
    base = torch.arange(0x3000, 0x3000 + n, dtype=torch.int32)
    assert 0x3000 + n < 0x7f80
    out = torch.stack([base[torch.randperm(n, generator=g)] for _ in range(rows)])
    return out.to(torch.int16).view(torch.bfloat16)


@pytest.mark.parametrize("H,G,n,k", [(2, 3, 4352, 672), (1, 2, 20000, 1000), (1, 2, 10003, 517), (1, 1, 77, 77), (1, 2, 5000, 0)])
def test_model_equals_scatter_topk_on_tie_free_rows(H, G, n, k):
    cs = _distinct_bf16_rows(H * G, n, seed=3).view(1, H, G, n)
    g = torch.Generator().manual_seed(4)
    static = torch.rand(1, H, G, n, generator=g) < 0.02
    groups = torch.tensor([True, False, True, True, False, True][:H * G]).view(1, H, G, 1)
    ref = torch.zeros(1, H, G, n, dtype=torch.bool)
    if k > 0:
        ref.scatter_(-1, cs.float().topk(k=k, dim=-1).indices, True)
    assert torch.equal(topk_mask_model(cs, k, groups, static), (ref & groups) | static)
    assert torch.equal(topk_mask_model(cs, k), ref)


def test_model_keys_are_order_preserving():
    vals = torch.tensor([-3.0, -1.0, -0.0078125, 0.0, 0.0078125, 1.0, 1.0078125, 300.0], dtype=torch.bfloat16)
    keys = bf16_keys(vals)
    assert (keys[1:] > keys[:-1]).all() and int(keys.min()) >= 0 and int(keys.max()) <= 0xFFFF


@pytest.mark.parametrize("n,k", [(4352, 300), (10003, 517), (20000, 1), (20000, 20000), (70000, 4900), (131072, 9175)])
def test_model_on_heavily_tied_rows_keeps_exactly_k_above_the_kth_value(n, k):
    g = torch.Generator().manual_seed(n + k)
    cs = (torch.randint(0, 40, (1, 1, 3, n), generator=g).float() / 8).to(torch.bfloat16)
    m = topk_mask_model(cs, k)
    x = cs.float()
    kth = x.sort(dim=-1, descending=True).values[..., k - 1:k]
    assert (m.sum(-1) == k).all()
    assert m[x > kth].all(), "every value above the k-th is kept"
    assert not m[x < kth].any(), "nothing below the k-th value is kept"
    # the stated tie order: among the columns equal to the k-th value, the kept ones come first in ((c % 4096) // 4, c) order
    c = torch.arange(n)
    rank = ((c % 4096) // 4) * (1 << 22) + c
    for r in range(3):
        tie = x[0, 0, r] == kth[0, 0, r]
        kept, left = rank[tie & m[0, 0, r]], rank[tie & ~m[0, 0, r]]
        assert kept.numel() >= 1 and (left.numel() == 0 or int(kept.max()) < int(left.min()))


def test_model_k_larger_than_n_and_inactive_rows():
    cs = (torch.randint(0, 40, (1, 1, 2, 1000), generator=torch.Generator().manual_seed(1)).float() / 8).to(torch.bfloat16)
    groups = torch.tensor([True, False]).view(1, 1, 2, 1)
    m = topk_mask_model(cs, 5000, groups, None)
    assert m[0, 0, 0].all() and not m[0, 0, 1].any()


def test_streaming_topk_mask_kernels_use_no_scratch(tmp_path):
    """topk_mask_stream_kernel (rows past the register form's 122 880 columns) re-reads its row instead of holding it: every
    instantiation -- ALIGNED, generic, PARTS -- compiles for gfx950 without spills and without scratch memory."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "indexed_io.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(CSRC, "indexed_io.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    names = re.findall(r"\.name:\s+(\S+)", text)
    scratch = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert len(names) == len(scratch) == len(spills)
    seen = 0
    for kname, sc, sp in zip(names, scratch, spills):
        if "topk_mask_stream_kernel" in kname:
            assert int(sp) == 0 and int(sc) == 0, f"{kname}: {sp} spills, {sc} bytes of scratch"
            seen += 1
    assert seen >= 3, names


def test_one_ceiling_in_library_operator_and_module():
    """common.h defines the longest row once; the Python constant next to ops.topk_mask carries the same number, the module gates on
    it, and it reaches the longest row mask_to_indices can still turn into indices (522 240)."""
    common = open(os.path.join(CSRC, "common.h")).read()
    m = re.search(r"#define\s+CHIPMUNK_TOPK_MASK_MAX_N\s+\((\d+)\s*\*\s*(\d+)\)", common)
    assert m, "CHIPMUNK_TOPK_MASK_MAX_N not found in common.h"
    ceiling = int(m.group(1)) * int(m.group(2))
    assert ceiling >= 522240
    assert ceiling <= 1024 * 512, "a thread's two packed u16 counters hold 512 keys"
    ns = {}
    src = open(os.path.join(ROOT, "chipmunk_amd", "ops", "indexed_io.py")).read()
    exec(re.search(r"^TOPK_MASK_MAX_N\s*=.*$", src, flags=re.M).group(0), ns)
    assert ns["TOPK_MASK_MAX_N"] == ceiling
    for fn in ("indexed_io.hip", "attn.hip"):
        host = open(os.path.join(CSRC, fn)).read()
        assert "CHIPMUNK_TOPK_MASK_MAX_N" in host
    module = open(os.path.join(ROOT, "chipmunk_amd", "modules", "attn.py")).read()
    assert module.count("ops.TOPK_MASK_MAX_N") == 2 and "122880" not in module
