"""mask -> ragged index rows (ops.mask_to_ragged_indices, attn.ragged_mask_to_indices): the same bits as the padded index tensor
followed by compact_indices, without that tensor -- as an operator, under the sparse attention, in its memory use and through
SparseDiffAttn over a schedule."""
import os

import pytest
import torch

from ragged_mask_cases import case_masks, expected_flat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (shape, forms): each the smallest that reaches its branch -- batch > 1; n % 32 != 0 with bool rows off 16-byte boundaries; packed rows
# off 4-byte boundaries; the shortest row; 98 blocks of 64 words (the scan of the block totals takes a second round of 64)
SHAPES = [((2, 2, 7, 1344), (False, True)), ((1, 2, 5, 1100), (False,)), ((1, 1, 6, 1096), (True,)), ((1, 1, 3, 8), (False, True)),
          ((1, 1, 3, 200000), (False, True))]
CASES = [(shape, packed) for shape, forms in SHAPES for packed in forms]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _old_pair(ops, mask, packed, shape, multiple_of, sorted_):
    if sorted_:
        inds, counts = ops.mask_to_sorted_indices(packed if packed is not None else mask, shape, multiple_of, 192)
    elif packed is not None:
        inds, counts = ops.packed_mask_to_indices(packed, shape, multiple_of, 192)
    else:
        inds, counts = ops.mask_to_indices(mask, multiple_of, 192)
    return (inds, counts) + tuple(ops.compact_indices(inds, counts))


@pytest.mark.parametrize("multiple_of", [1, 32, 128])
@pytest.mark.parametrize("sorted_", [True, False])
@pytest.mark.parametrize("shape,packed", CASES)
def test_operator_equals_the_padded_pair(dev, shape, packed, sorted_, multiple_of):
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd import ops
    n = shape[-1]
    for cpu_mask in case_masks(shape, multiple_of):
        mask = cpu_mask.to(dev)
        bits = ops.bitpack(mask)[0] if packed else None
        inds, counts, flat_old, off_old = _old_pair(ops, mask, bits, shape, multiple_of, sorted_)
        flat, offsets, got_counts = ops.mask_to_ragged_indices(bits if packed else mask, shape, multiple_of, 192, sorted_)
        assert got_counts.dtype == torch.int32 and got_counts.shape == counts.shape and torch.equal(got_counts, counts)
        assert offsets.dtype == torch.int64 and torch.equal(offsets, off_old)
        assert flat.dtype == torch.int32 and flat.numel() == flat_old.numel() == int(offsets[-1]) + 64
        total = int(offsets[-1])
        # every row: its first min(counts, n) entries are the padded row's, zeros from there to the next row; 64 zeros at the end
        assert torch.equal(flat[:total], expected_flat(inds.view(-1, inds.shape[-1]), counts, offsets, n))
        assert int(flat[total:].abs().sum()) == 0
        if n <= 1344:       # ... and the written-down layout (the operator's CPU path)
            ref = ops.mask_to_ragged_indices(cpu_mask, shape, multiple_of, 192, sorted_)
            assert all(torch.equal(a.cpu(), b) for a, b in zip((flat, offsets, got_counts), ref))


@pytest.mark.parametrize("sorted_", [True, False])
def test_sparse_attention_over_the_new_rows(dev, sorted_):
    """csp_attn_out_ragged over the operator's rows against csp_attn_out over the padded tensor, both signs; the mask has rows that keep
    nothing, everything (counts = 1408 > n = 1344: the padded row ends in undefined entries, the ragged one in zeros) and one key."""
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd import ops
    H, N = 2, 1344
    mask = case_masks((1, H, 7, N), 128, seed=5)[0].to(dev)
    g = torch.Generator(device=dev).manual_seed(16)
    q, k, v = [torch.randn(1, H, N, 128, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(3)]
    cache = torch.randn(1, N, H, 128, device=dev, dtype=torch.bfloat16, generator=g).permute(0, 2, 1, 3)
    packed, shape = ops.bitpack(mask)
    inds, counts, _, _ = _old_pair(ops, mask, packed, shape, 128, sorted_)
    flat, offsets, got_counts = ops.mask_to_ragged_indices(packed, shape, 128, 192, sorted_)
    assert int(counts.max()) == 1408 and int(counts.min()) == 0
    for scale in (1, -1):
        a = ops.csp_attn_out(q, k, v, cache, inds, counts, scale)
        b = ops.csp_attn_out_ragged(q, k, v, cache, flat, offsets, got_counts, scale)
        assert torch.equal(a, b), scale


def test_no_padded_tensor_is_allocated(dev):
    """[1, 2, 86, 16512] at 6 %: the padded index tensor is 11.4 MB.  The rise of the allocator's peak across one call stays under the
    result (4 bytes per entry of flat) + the per-row temporaries (counts, lengths, their running sum, offsets: 64 bytes a row) + 1 MiB
    of allocator rounding; across the old pair it exceeds the padded tensor, so the measurement sees what it claims to."""
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd import ops
    shape = (1, 2, 86, 16512)
    g = torch.Generator(device=dev).manual_seed(3)
    mask = torch.rand(shape, device=dev, generator=g) < 0.06
    packed, _ = ops.bitpack(mask)

    def rise(fn):
        fn()                                    # code objects loaded, allocator warm
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    new, (flat, offsets, counts) = rise(lambda: ops.mask_to_ragged_indices(packed, shape, 128, 192, True))
    old, _ = rise(lambda: ops.compact_indices(*ops.mask_to_sorted_indices(packed, shape, 128, 192)))
    rows, padded = counts.numel(), 4 * counts.numel() * 16512
    print(f"peak rise: new {new} B, old pair {old} B, padded tensor {padded} B, flat {4 * flat.numel()} B")
    assert old > padded
    assert new <= 4 * flat.numel() + 64 * rows + (1 << 20)


class _Calls:
    """Counting wrappers around the index operators of chipmunk_amd.ops (the module looks them up there at every call)."""
    NAMES = ("mask_to_indices", "packed_mask_to_indices", "mask_to_sorted_indices", "compact_indices", "mask_to_ragged_indices")

    def __init__(self, ops):
        self.ops, self.n, self.saved = ops, dict.fromkeys(self.NAMES, 0), {}

    def __enter__(self):
        for name in self.NAMES:
            self.saved[name] = fn = getattr(self.ops, name)

            def wrapper(*a, _fn=fn, _name=name, **kw):
                self.n[_name] += 1
                return _fn(*a, **kw)
            setattr(self.ops, name, wrapper)
        return self.n

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.ops, name, fn)


def _run_hunyuan_schedule(dev, ragged, resident, keep_offloaded=True, fused_residual=True, steps=13):
    """The 13-step, 5-layer (2 dense) HunyuanVideo schedule of tests/test_gpu_layout.py: full steps 0, 1 (mask) and 10 (mask recompute),
    sparse steps between.  Returns (layer outputs, layers that kept rows, bytes booked, operator calls)."""
    import chipmunk_amd  # noqa: F401
    from chipmunk_amd import ops
    from chipmunk_amd.modules import SparseDiffAttn
    from chipmunk_amd.util import config as cfgmod
    from chipmunk_amd.util import layer_counter as lc
    from chipmunk_amd.util.layer_counter import LayerCounter
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    cfgmod.reset_to_base()
    lc.singleton.__init__(0, 0)
    cfgmod.load_from_file(os.path.join(ROOT, "configs", "hunyuan_c3.yml"))
    cfg = cfgmod.GLOBAL_CONFIG
    cfg["steps"] = 50
    cfg["step_caching"]["is_enabled"] = False
    cfg["attn"]["token_major_output"] = True
    cfg["attn"]["keep_unpacked_indices"] = True
    cfg["attn"]["keep_unpacked_indices_offloaded"] = keep_offloaded
    cfg["attn"]["ragged_mask_to_indices"] = ragged
    cfg["attn"]["fused_residual"] = fused_residual
    cfg["offloading"]["keep_resident_if_fits"] = resident
    ot.gpu_tensors.clear()
    ops.manual_seed(9)
    torch.manual_seed(9)
    booked = ot._resident_bytes
    L, H, vid, txt = 5, 2, (4, 12, 16), 64
    N = vid[0] * vid[1] * vid[2] + txt
    g = torch.Generator(device=dev).manual_seed(21)
    q0, k0, v0, dq = [torch.randn(1, H, N, 128, device=dev, generator=g) for _ in range(4)]
    layers = []
    try:
        for _ in range(L):
            num, counter = LayerCounter.build_for_layer(is_attn_sparse=True)
            layers.append(SparseDiffAttn(num, counter))
        layers[0].initialize_static_mask(vid, txt, H, dev)
        outs = []
        with torch.no_grad(), _Calls(ops) as calls:
            for step in range(steps):
                q = (q0 + 0.03 * step * dq).to(torch.bfloat16)
                k, v = k0.to(torch.bfloat16), v0.to(torch.bfloat16)
                for li, layer in enumerate(layers):
                    if step > 0 or li > 0:
                        layer.storage.load_async_wait()
                    layers[(li + 1) % L].storage.load_async()
                    outs.append(layer(q, k, v).contiguous().clone())
                    layer.storage.complete_cur_layer()
        kept = [layer._unpacked[0] for layer in layers if layer._unpacked[0] is not None]
        for flat, _, counts, _, _ in kept:
            assert flat.numel() == int(((counts.flatten().long() + 31) // 32 * 32).sum()) + 64
        torch.cuda.synchronize()
        booked = ot._resident_bytes - booked
    finally:
        cfgmod.reset_to_base()
        lc.singleton.__init__(0, 0)
    return outs, len(kept), booked, calls


@pytest.mark.parametrize("resident,keep_offloaded,kept_layers", [(True, True, 3), (False, True, 3), (False, False, 0)],
                         ids=["resident", "offloaded_rows_kept", "offloaded_rows_not_kept"])
def test_module_schedule_is_unchanged_and_calls_no_padded_operator(dev, resident, keep_offloaded, kept_layers):
    off, kept_off, booked_off, calls_off = _run_hunyuan_schedule(dev, False, resident, keep_offloaded)
    on, kept_on, booked_on, calls_on = _run_hunyuan_schedule(dev, True, resident, keep_offloaded)
    assert len(on) == len(off) == 65
    for i, (a, b) in enumerate(zip(off, on)):
        assert torch.equal(a, b), f"layer call {i}"
    assert kept_on == kept_off == kept_layers and booked_on == booked_off
    assert (booked_on > 0) == (kept_layers > 0)
    assert calls_off["mask_to_ragged_indices"] == 0 and calls_off["mask_to_sorted_indices"] > 0
    assert (calls_off["compact_indices"] > 0) == (kept_layers > 0)
    assert [calls_on[name] for name in _Calls.NAMES[:4]] == [0, 0, 0, 0], calls_on
    # 3 sparse layers x 2 mask steps, and every sparse step (10 per sparse layer) of a layer whose rows were not kept
    assert calls_on["mask_to_ragged_indices"] == 6 + (0 if kept_layers else 30), calls_on


def test_module_without_fused_residual_keeps_the_old_operators(dev):
    ref, _, _, calls = _run_hunyuan_schedule(dev, True, True, fused_residual=False, steps=4)
    assert calls["mask_to_ragged_indices"] == 0 and calls["mask_to_sorted_indices"] > 0, calls
    same, _, _, _ = _run_hunyuan_schedule(dev, False, True, fused_residual=False, steps=4)
    assert all(torch.equal(a, b) for a, b in zip(ref, same))
