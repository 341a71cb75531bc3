"""time of chipmunk.split_heads_rownorm (Wan's q / k row-wide RMSNorm + rotary + head-major layout, q and k normalised and rotated with
fp32 weights, v copied) against (a) chipmunk.qkv_split_norm on the SAME tensor with per-head weights and the same tables -- another
function, but the same bytes through the per-head kernel -- and (b) the reference's torch sequence on the GPU (model.py:81-97, 49-78,
154-164: the operator's CPU path run on device tensors).  Device events around KB_ITERS calls, one process, every variant warmed up, the
variants alternated KB_ROUNDS times.  Algorithmic bytes: input + output + one read of the two tables.
Shapes: Wan 1.3B (n = 32760, 12 heads) at B = 1 and 2, Wan 14B 720p (n = 75600, 40 heads)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import chipmunk_amd
from chipmunk_amd import ops
from chipmunk_amd.ops import qkv as qkv_ops
dev = torch.device("cuda:0")
iters, rounds = int(os.environ.get("KB_ITERS", "20")), int(os.environ.get("KB_ROUNDS", "3"))
skip_torch = os.environ.get("KB_NO_TORCH", "0") == "1"
def t(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per call
def torch_sequence(x, heads, wq, wk, fc, fs):
    B, n, C = x.shape[0], x.shape[1], heads * 128
    out = []
    for p, w in enumerate((wq, wk)):
        y = qkv_ops._wan_rms_norm_reference(x[:, :, p * C:(p + 1) * C], w, 1e-6).view(B, n, heads, 128)
        out.append(qkv_ops._wan_rope_reference(y, fc, fs).permute(0, 2, 1, 3).to(torch.bfloat16))
    out.append(x[:, :, 2 * C:3 * C].reshape(B, n, heads, 128).permute(0, 2, 1, 3).to(torch.bfloat16).contiguous())
    return out
def shape(name, B, n, heads):
    g = torch.Generator(device=dev).manual_seed(n + heads)
    C = heads * 128
    x = (torch.randn(B, n, 3 * C, device=dev, generator=g) * 1.7).to(torch.bfloat16)
    wq, wk = [1 + 0.1 * torch.randn(C, device=dev, generator=g) for _ in range(2)]          # fp32: Wan's parameters
    hq, hk = [(1 + 0.1 * torch.randn(128, device=dev, generator=g)).to(torch.bfloat16) for _ in range(2)]
    ang = torch.rand(n, 64, device=dev, generator=g, dtype=torch.float64) * 6.28
    fc, fs = ang.cos().float().repeat_interleave(2, dim=1).contiguous(), ang.sin().float().repeat_interleave(2, dim=1).contiguous()
    nbytes = 2 * x.numel() * 2 + 2 * fc.numel() * 4
    variants = {"split_heads_rownorm": lambda: ops.split_heads_rownorm(x, heads, (wq, wk, None), (True, True, False), (True, True, False), 1e-6, fc, fs),
                "(a) qkv_split_norm, per head": lambda: [ops.qkv_split_norm(x[b], hq, hk, heads, 1e-6, fc, fs) for b in range(B)]}
    if not skip_torch:
        variants["(b) torch sequence"] = lambda: torch_sequence(x, heads, wq, wk, fc, fs)
    times = {k: [] for k in variants}
    for fn in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(t(fn, iters if not k.startswith("(b)") else max(2, iters // 10)))
    print(f"{name}: B={B} n={n} heads={heads}, {nbytes / 1e6:.1f} MB algorithmic, {iters} calls per figure")
    for k, v in times.items():
        med = sorted(v)[len(v) // 2]
        print(f"  {k:30s} us per call by round: {' '.join(f'{u:9.1f}' for u in v)}   median {med:9.1f} = {nbytes / med / 1e6:6.3f} TB/s   spread {max(v) - min(v):7.1f}")
    a = times["(a) qkv_split_norm, per head"]
    new = sorted(times["split_heads_rownorm"])[len(a) // 2]
    bound = sorted(a)[len(a) // 2] + (max(a) - min(a))
    print(f"  split_heads_rownorm median {new:.1f} us against (a) median + (a)'s spread = {bound:.1f} us: {'within' if new <= bound else 'ABOVE'}")
shape("Wan 1.3B", 1, 32760, 12)
shape("Wan 1.3B, cond + uncond", 2, 32760, 12)
shape("Wan 14B 720p", 1, 75600, 40)
