"""Launch times of the sparse-MLP selection with ``mlp.top_p``, the figures of DESIGN.md 4.3.  One GPU, device events, 5 launches after
a warm-up launch, bf16.

1. ``chipmunk_topk_delta_indices_p`` at top_p 0.5 / 0.75 / 0.9 against ``chipmunk_topk_delta_indices`` (KB_OTHER_LIB = path of a second
   libchipmunk_hip.so, e.g. built from the parent commit; default: this tree's, whose plain kernel is the parent's instruction for
   instruction) at ``[1, 34, 12288]`` (FLUX) and ``[1, 931, 12288]`` (HunyuanVideo): sparsity 0.7, 5 % random keys, multiple 256.  C ABI through
   ctypes on the null stream; the two operators alternate.  The cache is restored before every launch (the fused kernel writes it).
2. One SparseDiffMlp layer at FLUX's shape (M 4352, K 3072, F 12 288): a full step, then sparse steps on drifting inputs generated like
   tests/method_model.mlp_input (base + noise of a third of its size per step), every step making its selection: the time of the whole
   sparse call (block means, probe GEMM, selection, GEMM1 + scatter, GEMM2) and the mean stored count, with top_p off / 0.9 / 0.75 / 0.5.

The inputs are SYNTHETIC; what share of the columns a real model's deltas keep is not measured here."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import chipmunk_amd  # noqa: E402,F401
from chipmunk_amd import _native  # noqa: E402

dev = torch.device("cuda:0")
branch = _native.lib()
other = ctypes.CDLL(os.environ["KB_OTHER_LIB"]) if os.environ.get("KB_OTHER_LIB") else branch
vp, dbl = ctypes.c_void_p, ctypes.c_double
out = {}


def timed(fn, before=lambda: None, reps=5):
    before()
    fn()
    torch.cuda.synchronize()
    total = 0.0
    for _ in range(reps):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
    return total / reps


# ------------------------------------------------------------------------------------------------------------------ 1. the selection kernel
for rows in (34, 931):
    g = torch.Generator(device=dev).manual_seed(rows)
    f = 12288
    b = torch.randn(1, rows, f, device=dev, generator=g).to(torch.bfloat16)
    cache0 = (b.float() + (1.0 / 3.0) * torch.randn(1, rows, f, device=dev, generator=g)).to(torch.bfloat16)
    cache = cache0.clone()
    inds = torch.empty(1, rows, f, dtype=torch.int32, device=dev)
    counts = torch.empty(1, rows, dtype=torch.int32, device=dev)

    def plain():
        rc = other.chipmunk_topk_delta_indices(vp(b.data_ptr()), vp(cache.data_ptr()), 0, vp(inds.data_ptr()), vp(counts.data_ptr()), rows, f,
                                               dbl(0.7), 256, dbl(0.05), vp(0))
        assert rc == 0, rc

    def mass(top_p):
        rc = branch.chipmunk_topk_delta_indices_p(vp(b.data_ptr()), vp(cache.data_ptr()), 0, vp(inds.data_ptr()), vp(counts.data_ptr()), rows, f,
                                                  dbl(0.7), dbl(top_p), dbl(0.0), 256, dbl(0.05), vp(0))
        assert rc == 0, rc

    restore = lambda: cache.copy_(cache0)       # noqa: E731
    a, p = [], {0.5: [], 0.75: [], 0.9: []}
    for _ in range(3):          # alternate: the spread of each is the box's run-to-run spread
        a.append(timed(plain, restore) * 1e3)
        for top_p in p:
            p[top_p].append(timed(lambda: mass(top_p), restore) * 1e3)
    out[f"topk_delta_indices [1,{rows},{f}] us"] = a
    out[f"stored count [1,{rows},{f}] top_keys 0.3 (mean)"] = float(counts.float().mean())
    for top_p, v in p.items():
        out[f"topk_delta_indices_p [1,{rows},{f}] top_p {top_p} us"] = v
        restore()
        mass(top_p)
        out[f"stored count [1,{rows},{f}] top_p {top_p} (mean, min, max)"] = [float(counts.float().mean()), int(counts.min()), int(counts.max())]

# ------------------------------------------------------------------------------------------------------------------ 2. the sparse MLP step
from chipmunk_amd.modules import SparseDiffMlp  # noqa: E402
from chipmunk_amd.util import config as cfgmod  # noqa: E402
from chipmunk_amd.util.layer_counter import LayerCounter  # noqa: E402

M, K, F, STEPS = 4352, 3072, 12288, 7
gen = torch.Generator(device=dev).manual_seed(1)
base = torch.randn(1, M, K, device=dev, generator=gen)
xs = [(base + (1.0 / 3.0) * torch.randn(1, M, K, device=dev, generator=gen)).to(torch.bfloat16) for _ in range(STEPS)]
fc1, fc2 = torch.nn.Linear(K, F).to(dev).bfloat16(), torch.nn.Linear(F, K).to(dev).bfloat16()
for top_p in (0.0, 0.9, 0.75, 0.5):
    cfgmod.reset_to_base()
    cfg = cfgmod.GLOBAL_CONFIG
    cfg["offloading"]["global_disable_offloading"] = True
    cfg["mlp"].update(top_keys=0.3, random_keys=0.05, full_step_every=50, block_mask_cache=1, first_n_dense_layers=0, counts_multiple_of=256,
                      top_p=top_p, top_p_min_keys=0.0)
    mod = SparseDiffMlp(0, LayerCounter(1, 1), fc1, torch.nn.GELU(approximate="tanh"), fc2, 6)
    ms, stored = [], []
    with torch.no_grad():
        for step, x in enumerate(xs):
            if step:
                mod.storage.load_async_wait()
            mod.storage.load_async()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mod(x)
            e1.record()
            torch.cuda.synchronize()
            if step >= 2:        # step 0 is the full step, step 1 the warm-up sparse step
                ms.append(e0.elapsed_time(e1))
                stored.append(float(mod.storage.get_counts().float().mean()))
            mod.storage.complete_cur_layer()
    out[f"sparse MLP step M {M} K {K} F {F} top_p {top_p if top_p else 'off'} ms (5 steps)"] = [round(v, 3) for v in ms]
    out[f"mean stored count top_p {top_p if top_p else 'off'} (5 steps)"] = [round(v, 1) for v in stored]
cfgmod.reset_to_base()

for key, val in out.items():
    print(key, val)
if os.environ.get("KB_JSON"):
    with open(os.environ["KB_JSON"], "w") as fh:
        json.dump(out, fh, indent=1)
