"""time and peak memory of chipmunk.mask_to_ragged_indices (row counts -> offsets -> kept keys straight into ragged rows) against the pair
it replaces in SparseDiffAttn, chipmunk.mask_to_sorted_indices + chipmunk.compact_indices (padded [B, H, G, pad192(N)] tensor -> ragged
rows), on the same seeded bit-packed mask: 6 % of the keys per query group, the last two groups (the text groups) keeping every key.
Device events around KB_ITERS calls (each call holds its one host sync), one process, both variants warmed up and alternated KB_ROUNDS
times; the rise of the allocator's peak across one call of each.  Algorithmic bytes: the packed mask once + the ragged rows once.
Shapes: HunyuanVideo C3 [1, 24, 621, 119 056] and Wan2.1 1.3B [1, 12, 171, 32 760]."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import chipmunk_amd
from chipmunk_amd import ops
dev = torch.device("cuda:0")
iters, rounds = int(os.environ.get("KB_ITERS", "5")), int(os.environ.get("KB_ROUNDS", "3"))
def t(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per call
def peak_rise(fn):
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = fn(); torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before
def shape(name, H, G, n, density=0.06):
    g = torch.Generator(device=dev).manual_seed(n + H)
    heads = []
    for _ in range(H):                              # head by head: the bool mask of the C3 shape is 1.8 GB, its random source 7 GB
        m = torch.rand(G, n, device=dev, generator=g) < density
        m[-2:] = True
        heads.append(m)
    packed, shp = ops.bitpack(torch.stack(heads)[None])
    del heads, m
    variants = {"mask_to_sorted_indices + compact_indices": lambda: ops.compact_indices(*ops.mask_to_sorted_indices(packed, shp, 128, 192)),
                "mask_to_ragged_indices": lambda: ops.mask_to_ragged_indices(packed, shp, 128, 192, True)}
    old, new = [fn() for fn in variants.values()]
    assert torch.equal(old[1], new[1]) and old[0].numel() == new[0].numel()
    nbytes = packed.numel() + 4 * new[0].numel()
    del old, new
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(t(fn, iters))
    print(f"{name}: H={H} G={G} n={n}, packed mask {packed.numel() / 1e6:.1f} MB, {nbytes / 1e6:.1f} MB algorithmic, {iters} calls per figure")
    for k, v in times.items():
        med = sorted(v)[len(v) // 2]
        print(f"  {k:42s} us per call by round: {' '.join(f'{u:9.1f}' for u in v)}   median {med:9.1f} = {nbytes / med / 1e6:6.3f} TB/s   "
              f"spread {max(v) - min(v):7.1f}   peak rise {peak_rise(variants[k]) / 1e6:9.1f} MB")
    a = times["mask_to_sorted_indices + compact_indices"]
    new = sorted(times["mask_to_ragged_indices"])[len(a) // 2]
    bound = sorted(a)[len(a) // 2] + (max(a) - min(a))
    print(f"  mask_to_ragged_indices median {new:.1f} us against the pair's median + the pair's spread = {bound:.1f} us: {'within' if new <= bound else 'ABOVE'}")
shape("HunyuanVideo C3", 24, 621, 119056)
shape("Wan2.1 1.3B", 12, 171, 32760)
def mask_step_peak(H=24, vid=(33, 45, 80), txt=256):
    """allocator peak over one HunyuanVideo C3 mask step (step 1) of one SparseDiffAttn layer, attn.ragged_mask_to_indices off and on"""
    from chipmunk_amd.modules import SparseDiffAttn
    from chipmunk_amd.util import config as cfgmod, layer_counter as lc
    from chipmunk_amd.util.layer_counter import LayerCounter
    from chipmunk_amd.util.storage import offloaded_tensor as ot
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    N = vid[0] * vid[1] * vid[2] + txt
    g = torch.Generator(device=dev).manual_seed(1)
    q, k, v = [torch.randn(1, H, N, 128, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(3)]
    for ragged in (False, True):
        cfgmod.reset_to_base(); lc.singleton.__init__(0, 0)
        cfgmod.load_from_file(os.path.join(root, "configs", "hunyuan_c3.yml"))
        cfg = cfgmod.GLOBAL_CONFIG
        cfg["steps"] = 50; cfg["step_caching"]["is_enabled"] = False
        cfg["attn"]["first_n_dense_layers"] = 0
        cfg["attn"]["ragged_mask_to_indices"] = ragged
        cfg["offloading"]["keep_resident_if_fits"] = True
        ot.gpu_tensors.clear(); ops.manual_seed(9); torch.manual_seed(9)
        num, counter = LayerCounter.build_for_layer(is_attn_sparse=True)
        layer = SparseDiffAttn(num, counter)
        layer.initialize_static_mask(vid, txt, H, dev)
        with torch.no_grad():
            layer(q, k, v); layer.storage.complete_cur_layer()               # step 0: dense
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.max_memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); layer(q, k, v); e1.record(); torch.cuda.synchronize()   # step 1: mask step (first call: cold code objects)
        print(f"C3 mask step, one layer, attn.ragged_mask_to_indices={ragged}: allocator peak {torch.cuda.max_memory_allocated() / 1e9:.2f} GB, "
              f"{(torch.cuda.max_memory_allocated() - before) / 1e9:.2f} GB above the state before the step; {e0.elapsed_time(e1):.1f} ms (cold)")
        layer.release_kept_indices(); del layer
        cfgmod.reset_to_base(); lc.singleton.__init__(0, 0)
mask_step_peak()
