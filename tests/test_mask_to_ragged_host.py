"""Host checks for mask -> ragged index rows: the torch statement of the layout (the CPU path of ops.mask_to_ragged_indices) against
the oracle's mask_to_indices, the C entries' refusals (nothing is launched here), and the compiled kernels' resource use."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from ragged_mask_cases import case_masks, expected_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chipmunk_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SHAPES = [(2, 2, 7, 1344), (1, 2, 5, 1100), (1, 1, 6, 1096), (1, 1, 3, 8)]


def _check_layout(flat, offsets, counts, n, pad_n):
    width = (counts.flatten().long().clamp(max=pad_n) + 31) // 32 * 32
    assert offsets.dtype == torch.int64 and int(offsets[0]) == 0 and torch.equal(offsets[1:], width.cumsum(0))
    assert flat.dtype == torch.int32 and flat.numel() == int(offsets[-1]) + 64 and int(flat[int(offsets[-1]):].abs().sum()) == 0


@pytest.mark.parametrize("multiple_of", [1, 32, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_path_in_reference_order_equals_the_oracle(shape, multiple_of):
    import oracle
    from chipmunk_amd import ops
    n, pad_n = shape[-1], (shape[-1] + 191) // 192 * 192
    for mask in case_masks(shape, multiple_of):
        inds, counts = oracle.mask_to_indices(mask, multiple_of, 192)
        flat, offsets, got_counts = ops.mask_to_ragged_indices(mask, mask.shape, multiple_of, 192, sorted=False)
        assert got_counts.dtype == torch.int32 and torch.equal(got_counts, counts)
        _check_layout(flat, offsets, counts, n, pad_n)
        # row by row: the first min(counts, n) entries are the oracle's, zeros behind them
        assert torch.equal(flat[:-64], expected_flat(inds.view(-1, pad_n), counts, offsets, n))
        if n % 8 == 0:      # the bit-packed form of the same mask
            packed, shp = ops.bitpack(mask)
            again = ops.mask_to_ragged_indices(packed, shp, multiple_of, 192, sorted=False)
            assert all(torch.equal(a, b) for a, b in zip(again, (flat, offsets, got_counts)))


@pytest.mark.parametrize("multiple_of", [1, 32, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_path_sorted_is_the_same_set_ascending(shape, multiple_of):
    from chipmunk_amd import ops
    n = shape[-1]
    for mask in case_masks(shape, multiple_of):
        ref, off_ref, cnt_ref = ops.mask_to_ragged_indices(mask, mask.shape, multiple_of, 192, sorted=False)
        flat, offsets, counts = ops.mask_to_ragged_indices(mask, mask.shape, multiple_of, 192)       # sorted is the default
        assert torch.equal(offsets, off_ref) and torch.equal(counts, cnt_ref) and flat.numel() == ref.numel()
        kept = mask.view(-1, n).sum(dim=1)
        for r in range(kept.numel()):
            o, k, end = int(offsets[r]), int(kept[r]), int(offsets[r + 1])
            assert torch.equal(flat[o:o + k], ref[o:o + k].sort().values), r
            assert torch.equal(flat[o:o + k], torch.nonzero(mask.view(-1, n)[r]).flatten().to(torch.int32)), r
            assert torch.equal(flat[o + k:end], ref[o + k:end]), f"row {r}: the same padding columns and zeros"


def _entries():
    from chipmunk_amd import _native
    lib = _native.lib()
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.chipmunk_mask_row_counts.argtypes = [P, I, P, P, L, I, I, I, P]
    lib.chipmunk_mask_to_ragged_indices.argtypes = [P, I, I, P, P, L, I, I, P]

    def counts(mask=16, packed=0, counts=16, lengths=16, rows=4, n=1344, pad_n=1344, multiple_of=128):
        return lib.chipmunk_mask_row_counts(mask, packed, counts, lengths, rows, n, pad_n, multiple_of, None)

    def emit(mask=16, packed=0, sorted=1, offsets=16, flat=16, rows=4, n=1344, multiple_of=128):
        return lib.chipmunk_mask_to_ragged_indices(mask, packed, sorted, offsets, flat, rows, n, multiple_of, None)
    return _native, counts, emit


def test_new_entries_are_exported_and_refuse_bad_arguments():
    """Every refusal comes before any HIP call (the pointers here point nowhere), with a message; no rows, no launch."""
    native, counts, emit = _entries()
    assert {"chipmunk_mask_row_counts", "chipmunk_mask_to_ragged_indices"} <= set(native.SYMBOLS)
    for fn, pointers in ((counts, ("mask", "counts", "lengths")), (emit, ("mask", "offsets", "flat"))):
        for name in pointers:
            assert fn(**{name: None}) == 1 and "null" in native.last_error(), name
        assert fn(packed=1, n=1100) == 1 and "multiple of 8" in native.last_error()
        assert fn(multiple_of=0) == 1 and "multiple_of=0" in native.last_error()
        assert fn(n=0) == 1 and "n=0" in native.last_error()
        assert fn(rows=1 << 31) == 1 and "too many rows" in native.last_error()
        assert fn(n=1 << 21, **({"pad_n": 1 << 21} if fn is counts else {})) == 1 and "LDS" in native.last_error()
        assert fn(rows=0) == 0
    assert counts(pad_n=1343) == 1 and "pad_n=1343" in native.last_error()
    # the reference order needs more LDS per column than the ascending one: a row the one takes and the other refuses
    assert emit(n=600000, sorted=1, rows=0) == 0
    assert emit(n=600000, sorted=0, rows=0) == 1 and "LDS" in native.last_error()


def test_new_kernels_do_not_spill(tmp_path):
    """mask_row_counts_kernel (2 forms) and the ragged forms of mask_to_indices_kernel (4): no VGPR spills, no scratch, from the metadata
    of the gfx950 code object."""
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
    seen = set()
    for kname, sc, sp in zip(names, scratch, spills):
        if "mask_row_counts_kernel" in kname or re.search(r"mask_to_indices_kernelILb[01]ELb[01]ELb1E", kname):
            assert int(sp) == 0 and int(sc) == 0, f"{kname}: {sp} spills, {sc} bytes of scratch"
            seen.add(kname)
    assert len(seen) == 6, seen
