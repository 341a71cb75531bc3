"""cost of the streaming form of the top-k mask kernel against the register form: nanoseconds per column of ops.topk_mask on
KB_ROWS rows (default 2048 = 8 per CU) of random bf16, random part 1 %, a 0.2 % static mask of one row broadcast by stride --
register form at n = 122 880 (its longest row), streaming form at the same n (option topk_mask_stream = 1) and at KB_N
(default 245 760)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import chipmunk_amd
from chipmunk_amd import ops, _native
dev = torch.device("cuda:0")
rows, n_long = int(os.environ.get("KB_ROWS", "2048")), int(os.environ.get("KB_N", "245760"))
def t(fn, n=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
def run(n, stream):
    g = torch.Generator(device=dev).manual_seed(3)
    cs = torch.randn(1, 1, rows, n, device=dev, generator=g).to(torch.bfloat16)
    gr = torch.ones(1, 1, rows, 1, dtype=torch.bool, device=dev)
    k = 128 * round(0.05 * n / 128)
    _native.set_option("topk_mask_stream", stream)
    try:
        ms = t(lambda: ops.topk_mask(cs, k, 0.01, gr, None))
    finally:
        _native.set_option("topk_mask_stream", 0)
    form = "streaming" if stream or n > 122880 else "register"
    print(f"{form:9s} n={n:6d} rows={rows} k={k}: {ms:.3f} ms = {ms * 1e6 / (rows * n):.4f} ns per column, {ms * 1e3 / rows * 256:.1f} us per row and CU")
    return ms
ops.manual_seed(1)
run(122880, 0)
run(122880, 1)
run(n_long, 0)
