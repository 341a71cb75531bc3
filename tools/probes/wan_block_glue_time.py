"""time of chipmunk.residual_ln_modulate_f32 (Wan's block glue: fp32 residual + LayerNorm + modulate / affine in one pass) against the
reference's torch sequence on the GPU (model.py:100-110, 324-334: the operator's CPU path run on device tensors), for the four uses of a
block: (1) norm1 + modulate of the stream alone, (2) gated residual + affine norm3, (3) ungated residual + norm2 + modulate, (4) gated
residual + the next block's norm1 + modulate.  Device events around KB_ITERS calls (a fifth as many of the torch sequence), one process,
every variant warmed up, KB_ROUNDS rounds with the two orders alternating.  Algorithmic bytes: 12 * rows * C with y (x fp32 in and out,
y and xm bf16), 6 * rows * C without.  The outputs of the two are compared once per use: the stream bit for bit, xm by its largest
difference.  Shapes: Wan 1.3B (L = 32760, C = 1536) and Wan 14B (C = 5120) at B = 1 and 2 (cond + uncond)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import chipmunk_amd
from chipmunk_amd import ops
from chipmunk_amd.ops import qkv as qkv_ops
dev = torch.device("cuda:0")
iters, rounds = int(os.environ.get("KB_ITERS", "50")), int(os.environ.get("KB_ROUNDS", "5"))
L = int(os.environ.get("KB_L", "32760"))
def t(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per call
def shape(name, B, C):
    g = torch.Generator(device=dev).manual_seed(B * 10000 + C)
    x = torch.randn(B, L, C, device=dev, generator=g) * 2 + 0.3
    y = torch.randn(B, L, C, device=dev, generator=g).to(torch.bfloat16)
    e = torch.randn(B, 6, C, device=dev, generator=g)                                   # fp32, one set per sequence (model.py:317-320)
    gate, shift, scale = e[:, 2:3].contiguous(), e[:, 0:1].contiguous(), e[:, 1:2].contiguous()
    w, b = 1 + 0.3 * torch.randn(C, device=dev, generator=g), torch.randn(C, device=dev, generator=g)
    uses = {"(1) norm1 + modulate": dict(y=None, gate=None, shift=shift, scale=scale, weight=None, bias=None),
            "(2) gated residual + affine norm3": dict(y=y, gate=gate, shift=None, scale=None, weight=w, bias=b),
            "(3) residual + norm2 + modulate": dict(y=y, gate=None, shift=shift, scale=scale, weight=None, bias=None),
            "(4) gated residual + norm1 + modulate": dict(y=y, gate=gate, shift=shift, scale=scale, weight=None, bias=None)}
    print(f"{name}: B={B} L={L} C={C}, {iters} calls per figure ({max(2, iters // 5)} of the torch sequence), {rounds} rounds")
    for use, kw in uses.items():
        nbytes = (12 if kw["y"] is not None else 6) * B * L * C
        variants = {"operator": lambda: ops.residual_ln_modulate_f32(x, **kw, eps=1e-6),
                    "torch": lambda: qkv_ops._wan_block_glue_reference(x, eps=1e-6, **kw)}
        (ox, om), (tx, tm) = variants["operator"](), variants["torch"]()
        torch.cuda.synchronize()
        same_x = kw["y"] is None or torch.equal(ox, tx)
        diff = float((om.float() - tm.float()).abs().max())
        del ox, om, tx, tm
        for fn in variants.values():
            fn(); fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for r in range(rounds):
            for k in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
                times[k].append(t(variants[k], iters if k == "operator" else max(2, iters // 5)))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        print(f"  {use}: {nbytes / 1e6:.0f} MB algorithmic; stream {'bit-equal' if same_x else 'DIFFERS'}, largest |xm difference| {diff:.4g}")
        for k, v in times.items():
            print(f"    {k:9s} us per call by round: {' '.join(f'{u:9.1f}' for u in v)}   median {med[k]:9.1f} = {nbytes / med[k] / 1e6:6.3f} TB/s   spread {max(v) - min(v):7.1f}")
        print(f"    torch / operator = {med['torch'] / med['operator']:.2f}; slowest operator round {max(times['operator']):.1f} us against the fastest torch round "
              f"{min(times['torch']):.1f} us: {'faster in every round' if max(times['operator']) < min(times['torch']) else 'NOT faster in every round'}")
for name, B, C in (("Wan 1.3B", 1, 1536), ("Wan 1.3B, cond + uncond", 2, 1536), ("Wan 14B", 1, 5120), ("Wan 14B, cond + uncond", 2, 5120)):
    shape(name, B, C)
    torch.cuda.empty_cache()
