#!/usr/bin/env python
"""Per-kernel micro-benchmark at the BASELINE shapes: back-to-back launches inside one HIP-event bracket, so the
number is kernel time (comparable with rocprofv3's average duration), not host launch latency.

usage: python tools/kbench.py [mm1 mm1s mm1_act mm1_glu mm1_glu_fp8 mm2 mm2_w8 mm2_w8_wan mm1_w8 mm1_w8_wan mm1_glu_w8 w8_probe w8_probe_wan w8_probe_hunyuan scatter fp8_wan fp8_rs_wan fp8_wan_groups mm1s_groups to_groups mm2_wan fp8_wan_ragged fp8_wan_ragged_pitched mm2_wan_ragged mm1s_hunyuan mm2_hunyuan csp_flux csp_hunyuan dense_flux colsum_flux maskstep_hunyuan topk m2i copy group_delta] [--variants 0,1,2]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import chipmunk_amd  # noqa: E402,F401
from chipmunk_amd import _native  # noqa: E402

dev = torch.device("cuda:0")


_warm = {"done": False}


def warm_gpu(ms=300.0):
    """Bring the clocks up before the first measurement (the first kernel timed in a cold process reads ~10 % slow)."""
    if _warm["done"]:
        return
    a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    while True:
        for _ in range(20):
            a @ a
        t1.record()
        t1.synchronize()
        if t0.elapsed_time(t1) > ms:
            break
    _warm["done"] = True


def timeit(fn, reps=20, warm=3, rounds=3):
    """Median over `rounds` brackets of `reps` back-to-back launches each."""
    warm_gpu()
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) / reps)
    return sorted(out)[len(out) // 2]  # ms


def rand_rows(G, F, count, g):
    inds = torch.empty(G, F, dtype=torch.int32, device=dev)
    for i in range(G):
        inds[i] = torch.randperm(F, device=dev, generator=g).to(torch.int32)
    inds[:, :count] = inds[:, :count].sort(dim=1).values
    return inds.contiguous()


def batch_env():
    """(KB_BATCH, KB_BATCH_LOOP): sequences per call, and whether a call is one batched launch (default) or a loop of launches"""
    return int(os.environ.get("KB_BATCH", "1")), os.environ.get("KB_BATCH_LOOP") == "1"


def batch_tag(B, loop):
    return "" if B == 1 else f" batch={B} as {B} launches" if loop else f" batch={B} in one launch"


def bench_mlp(which, variants, M=4352, K=3072, F=12288, keep=4096):
    """KB_LAYERS=n rotates n independent sets of weights / caches / outputs per launch (n = 8: 1.7 GB, far beyond the
    256 MB Infinity Cache) -- the in-pipeline condition, where every layer's weights come from HBM.  Default 1: the
    same buffers every launch, which the Infinity Cache then serves.
    KB_BATCH=n: n sequences of M rows (operands [n, M, .], cache [n, F, M], indices [n, G, F]) in ONE batched launch per call;
    with KB_BATCH_LOOP=1 the same operands as n back-to-back single-sequence launches on the slices.  The time is per call: all n."""
    g = torch.Generator(device=dev).manual_seed(0)
    L = int(os.environ.get("KB_LAYERS", "1"))
    B, loop = batch_env()
    a = torch.randn(B, M, K, device=dev, dtype=torch.bfloat16, generator=g)
    bias = torch.zeros(F, device=dev, dtype=torch.bfloat16)
    sets = []
    for _ in range(L):
        w1 = (torch.randn(F, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        cache = torch.randn(B, F, M, device=dev, dtype=torch.bfloat16, generator=g)
        packed = torch.randn(B, M, F, device=dev, dtype=torch.bfloat16, generator=g) * 0.1
        w2t = (torch.randn(F, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        out = torch.zeros(B, M, K, device=dev, dtype=torch.bfloat16)
        sets.append((w1, cache, packed, w2t, out))
    G = (M + 127) // 128      # (a token count that is no multiple of 128: the last group is short)
    inds = rand_rows(B * G, F, keep, g)
    if os.environ.get("KB_SAME_INDICES") == "1":   # every group selects the same columns: upper bound of L2 sharing
        inds[:] = inds[0:1]
    inds = inds.view(B, G, F)
    counts = torch.full((B, G), keep, dtype=torch.int32, device=dev)
    flops = 2.0 * B * M * K * keep
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % L
        return sets[state["i"]]

    def each(op):
        """op on the operands of every launch of one call: the whole batch at once, or one sequence at a time"""
        for b in (range(B) if loop or B == 1 else [slice(None)]):
            op(b)

    def run_mm1():
        w1, cache, packed, _, _ = nxt()
        each(lambda b: torch.ops.chipmunk.csp_mlp_mm1(a[b], w1, packed[b], bias, cache[b], inds[b], counts[b]))

    def run_mm1s():
        w1, cache, packed, _, _ = nxt()
        each(lambda b: torch.ops.chipmunk.csp_mlp_mm1_scatter(a[b], w1, packed[b], bias, cache[b], inds[b], counts[b]))

    def run_mm2():
        _, _, packed, w2t, out = nxt()
        each(lambda b: torch.ops.chipmunk.csp_mlp_mm2(packed[b], w2t, inds[b], counts[b], out[b]))

    def run_scatter():
        _, cache, packed, _, _ = nxt()
        torch.ops.chipmunk.csp_scatter_add(packed[:1], cache[:1], inds[:1], counts[:1], 6)

    tag = f"(M={M} K={K} keep={keep} layers={L}{batch_tag(B, loop)})"
    for v in variants:
        if which == "mm1":
            _native.set_option("mm1_variant", v)
            ms = timeit(run_mm1)
            print(f"mm1   variant {v}: {ms*1e3:8.1f} us  {flops/ms/1e9:7.1f} TFLOP/s   {tag}")
        elif which == "mm1s":
            _native.set_option("mm1_variant", v)
            ms = timeit(run_mm1s)
            print(f"mm1+scatter v{v}: {ms*1e3:8.1f} us  {flops/ms/1e9:7.1f} TFLOP/s   {tag}")
        elif which == "mm2":
            _native.set_option("mm2_variant", v)
            ms = timeit(run_mm2)
            print(f"mm2   variant {v}: {ms*1e3:8.1f} us  {flops/ms/1e9:7.1f} TFLOP/s   {tag}")
        elif which == "scatter":
            ms = timeit(run_scatter)
            byts = 3.0 * M * keep * 2
            print(f"scatter_add    : {ms*1e3:8.1f} us  {byts/ms/1e6:7.1f} GB/s algorithmic")
            break
    _native.set_option("mm1_variant", 0)
    _native.set_option("mm2_variant", 0)


def bench_mm1_glu(M=4352, K=3072, F=12288, keep=3840, act="silu"):
    """The gated GEMM1 (csp_mlp_mm1_glu, 30 % of the columns kept) against the ungated csp_mlp_mm1 with twice the kept columns over a
    [2F, K] weight: equal matrix work and equal gathered weight bytes, the ungated launch reads a cache block and writes packed deltas
    of twice the width.  Same process, the two alternating (KB_ROUNDS pairs, default 5); per launch the median bracket of `timeit`,
    then the median and the range over the rounds.  KB_GLU_UPDATE=1 times the scatter forms of both."""
    g = torch.Generator(device=dev).manual_seed(0)
    upd = os.environ.get("KB_GLU_UPDATE") == "1"
    a = torch.randn(M, K, device=dev, dtype=torch.bfloat16, generator=g)
    w = (torch.randn(2 * F, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)      # gated: its halves; ungated: the whole
    bias = torch.zeros(2 * F, device=dev, dtype=torch.bfloat16)
    cache = torch.randn(2 * F, M, device=dev, dtype=torch.bfloat16, generator=g)
    packed = torch.empty(M, 2 * F, device=dev, dtype=torch.bfloat16)
    G = (M + 127) // 128
    inds1, inds2 = rand_rows(G, F, keep, g), rand_rows(G, 2 * F, 2 * keep, g)
    c1, c2 = torch.full((G,), keep, dtype=torch.int32, device=dev), torch.full((G,), 2 * keep, dtype=torch.int32, device=dev)
    packed1 = packed[:, :F].contiguous()
    ungated = torch.ops.chipmunk.csp_mlp_mm1_scatter if upd else torch.ops.chipmunk.csp_mlp_mm1

    def run_glu():
        torch.ops.chipmunk.csp_mlp_mm1_glu(a, w[:F], w[F:], packed1, None, None, cache[:F], inds1, c1, act, upd)

    def run_ungated():
        ungated(a, w, packed, bias, cache, inds2, c2)
    rounds = int(os.environ.get("KB_ROUNDS", "5"))
    t = {"glu": [], "mm1": []}
    for _ in range(rounds):
        t["glu"].append(timeit(run_glu) * 1e3)
        t["mm1"].append(timeit(run_ungated) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    flops = 2.0 * M * K * 2 * keep
    tag = f"(M={M} K={K} F={F} keep={keep} {'scatter' if upd else 'update off'}, {rounds} alternating rounds)"
    print(f"mm1_glu {act:9s}: {med['glu']:8.1f} us  [{min(t['glu']):.1f} .. {max(t['glu']):.1f}]  {flops/med['glu']/1e6:7.1f} TFLOP/s   {tag}")
    print(f"mm1 2x keep, 2F : {med['mm1']:8.1f} us  [{min(t['mm1']):.1f} .. {max(t['mm1']):.1f}]  {flops/med['mm1']/1e6:7.1f} TFLOP/s")
    print(f"mm1_glu / mm1   : {med['glu'] / med['mm1']:8.3f}")


def bench_mm1_act(M=4352, K=3072, F=12288, keep=3840):
    """The ungated GEMM1 with the activation as an argument (csp_mlp_mm1_act, scatter form, with a bias and -- tanh-GELU -- without one) at
    the FLUX MLP shape, 30 % of the columns kept, against csp_mlp_mm1_scatter on the same operands: the same tile code, the epilogue's
    activation apart.  Same process, all launches alternating (KB_ROUNDS rounds, default 5); per launch the median bracket of `timeit`,
    then the median and the range over the rounds."""
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.randn(M, K, device=dev, dtype=torch.bfloat16, generator=g)
    w = (torch.randn(F, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    bias = (torch.randn(F, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    cache = torch.randn(F, M, device=dev, dtype=torch.bfloat16, generator=g)
    packed = torch.empty(M, F, device=dev, dtype=torch.bfloat16)
    G = (M + 127) // 128
    inds, counts = rand_rows(G, F, keep, g), torch.full((G,), keep, dtype=torch.int32, device=dev)
    ops = torch.ops.chipmunk
    runs = {"mm1_scatter (tanh-GELU)": lambda: ops.csp_mlp_mm1_scatter(a, w, packed, bias, cache, inds, counts)}
    for act in ("gelu_tanh", "silu", "gelu"):
        runs[f"mm1_act {act}"] = lambda act=act: ops.csp_mlp_mm1_act(a, w, packed, bias, cache, inds, counts, act, True)
    runs["mm1_act gelu_tanh, no bias"] = lambda: ops.csp_mlp_mm1_act(a, w, packed, None, cache, inds, counts, "gelu_tanh", True)
    rounds = int(os.environ.get("KB_ROUNDS", "5"))
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            t[k].append(timeit(fn) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    flops = 2.0 * M * K * keep
    print(f"(M={M} K={K} F={F} keep={keep} scatter forms, {rounds} alternating rounds)")
    for k in runs:
        print(f"{k:28s}: {med[k]:8.1f} us  [{min(t[k]):.1f} .. {max(t[k]):.1f}]  {flops/med[k]/1e6:7.1f} TFLOP/s   x {med[k] / med['mm1_scatter (tanh-GELU)']:.3f}")


def bench_mm1_glu_fp8(M=32768, K=1536, F=8960, keep=2816, act="silu"):
    """The gated fp8 GEMM1 (csp_mlp_mm1_glu_fp8) at the Wan fp8 shape, 30 % of the columns kept (rounded to 256), against the ungated
    csp_mlp_mm1_fp8 with twice the kept columns over a [2F, K] e4m3 weight: equal matrix work and equal gathered weight bytes, as
    bench_mm1_glu.  Same process, the two alternating (KB_ROUNDS pairs, default 5); per launch the median bracket of `timeit`, then the
    median and the range over the rounds.  KB_GLU_UPDATE=1 times the scatter forms of both."""
    g = torch.Generator(device=dev).manual_seed(0)
    upd = os.environ.get("KB_GLU_UPDATE") == "1"
    a8 = (torch.randn(M, K, device=dev, generator=g) * 16).clamp(-448, 448).to(torch.float8_e4m3fn)
    w8 = (torch.randn(2 * F, K, device=dev, generator=g) * 0.02 * 512).clamp(-448, 448).to(torch.float8_e4m3fn)   # gated: its halves
    sa, sb, sb2 = (torch.tensor([v], device=dev) for v in (1 / 16.0, 1 / 512.0, 1 / 256.0))
    bias = torch.zeros(2 * F, device=dev, dtype=torch.bfloat16)
    cache = torch.randn(2 * F, M, device=dev, dtype=torch.bfloat16, generator=g)
    packed = torch.empty(M, 2 * F, device=dev, dtype=torch.bfloat16)
    G = (M + 127) // 128
    inds1, inds2 = rand_rows(G, F, keep, g), rand_rows(G, 2 * F, 2 * keep, g)
    c1, c2 = torch.full((G,), keep, dtype=torch.int32, device=dev), torch.full((G,), 2 * keep, dtype=torch.int32, device=dev)
    packed1 = packed[:, :F].contiguous()

    def run_glu():
        torch.ops.chipmunk.csp_mlp_mm1_glu_fp8(a8, w8[:F], w8[F:], packed1, None, None, cache[:F], inds1, c1, sa, sb, sb2, act, upd)

    def run_ungated():
        if upd:
            torch.ops.chipmunk.csp_mlp_mm1_fp8_scatter(a8, w8, packed, bias, cache, inds2, c2, sa, sb)
        else:
            torch.ops.chipmunk.csp_mlp_mm1_fp8(a8, w8, packed, bias, cache, inds2, c2, sa, sb, False)
    rounds = int(os.environ.get("KB_ROUNDS", "5"))
    t = {"glu": [], "mm1": []}
    for _ in range(rounds):
        t["glu"].append(timeit(run_glu) * 1e3)
        t["mm1"].append(timeit(run_ungated) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    flops = 2.0 * M * K * 2 * keep
    tag = f"(M={M} K={K} F={F} keep={keep} {'scatter' if upd else 'update off'}, {rounds} alternating rounds)"
    print(f"mm1_glu_fp8 {act:9s}: {med['glu']:8.1f} us  [{min(t['glu']):.1f} .. {max(t['glu']):.1f}]  {flops/med['glu']/1e6:7.1f} TFLOP/s   {tag}")
    print(f"mm1_fp8 2x keep, 2F : {med['mm1']:8.1f} us  [{min(t['mm1']):.1f} .. {max(t['mm1']):.1f}]  {flops/med['mm1']/1e6:7.1f} TFLOP/s")
    print(f"mm1_glu_fp8 / mm1_fp8: {med['glu'] / med['mm1']:7.3f}")


def bench_mm2_w8(M=4352, F=12288, N2=3072, keep=3840):
    """The weight-only fp8 GEMM2 (csp_mlp_mm2_w8: e4m3 rows of fc2^T) against the bf16 csp_mlp_mm2 on the same packed deltas, index lists
    and shape.  Same process, the two alternating (KB_ROUNDS pairs, default 5); per launch the median bracket of `timeit` (20 launches,
    clocks warmed), then the median and the range over the rounds.  KB_LAYERS=n rotates n sets of weights / deltas / outputs (n = 8: the
    weight rows come from HBM, not from the Infinity Cache)."""
    g = torch.Generator(device=dev).manual_seed(0)
    L = int(os.environ.get("KB_LAYERS", "1"))
    sets = []
    for _ in range(L):
        w = torch.randn(F, N2, device=dev, generator=g) * 0.02
        w8 = (w * 512).clamp(-448, 448).to(torch.float8_e4m3fn)
        packed = torch.randn(M, F, device=dev, dtype=torch.bfloat16, generator=g) * 0.1
        sets.append((w.to(torch.bfloat16), w8, packed, torch.zeros(M, N2, device=dev, dtype=torch.bfloat16)))
    sb = torch.tensor([1 / 512.0], device=dev)
    G = (M + 127) // 128
    inds = rand_rows(G, F, keep, g)
    counts = torch.full((G,), keep, dtype=torch.int32, device=dev)
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % L
        return sets[state["i"]]

    def run_w8():
        _, w8, packed, out = nxt()
        torch.ops.chipmunk.csp_mlp_mm2_w8(packed, w8, sb, inds, counts, out)

    def run_bf16():
        w16, _, packed, out = nxt()
        torch.ops.chipmunk.csp_mlp_mm2(packed, w16, inds, counts, out)
    rounds = int(os.environ.get("KB_ROUNDS", "5"))
    t = {"w8": [], "bf16": []}
    for _ in range(rounds):
        t["w8"].append(timeit(run_w8) * 1e3)
        t["bf16"].append(timeit(run_bf16) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    flops = 2.0 * M * N2 * keep
    tag = f"(M={M} F={F} N2={N2} keep={keep} layers={L}, {rounds} alternating rounds)"
    print(f"mm2_w8  e4m3 rows: {med['w8']:8.1f} us  [{min(t['w8']):.1f} .. {max(t['w8']):.1f}]  {flops/med['w8']/1e6:7.1f} TFLOP/s   {tag}")
    print(f"mm2     bf16 rows: {med['bf16']:8.1f} us  [{min(t['bf16']):.1f} .. {max(t['bf16']):.1f}]  {flops/med['bf16']/1e6:7.1f} TFLOP/s")
    print(f"mm2_w8 / mm2     : {med['w8'] / med['bf16']:8.3f}")


def bench_mm1_w8(M=4352, K=3072, F=12288, keep=3840):
    """The weight-only fp8 GEMM1 with its scatter-add (csp_mlp_mm1_w8: e4m3 rows of fc1, bf16 activations) against the bf16
    csp_mlp_mm1_scatter (`mm1s`) on the same activations, index lists and shape.  Same process, the two alternating (KB_ROUNDS pairs,
    default 5); per launch the median bracket of `timeit` (20 launches, clocks warmed), then the median and the range over the rounds.
    KB_LAYERS=n rotates n sets of weights / caches / outputs (n = 8: the weight rows come from HBM).  KB_W8_SCALES=row: one scale per fc1
    row instead of one number.  Also times the selecting step's block-mean probe fc1(block_mean(x)) through W8Linear.forward (the whole
    weight widened per call) against the bf16 nn.Linear."""
    from chipmunk_amd.modules import W8Linear
    g = torch.Generator(device=dev).manual_seed(0)
    L = int(os.environ.get("KB_LAYERS", "1"))
    rows = os.environ.get("KB_W8_SCALES", "tensor") == "row"
    G = (M + 127) // 128
    ldc = (M + 7) // 8 * 8
    sets = []
    for _ in range(L):
        w = torch.randn(F, K, device=dev, generator=g) * 0.02
        w8 = (w * 512).clamp(-448, 448).to(torch.float8_e4m3fn)
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, generator=g) * 0.5
        bias = torch.randn(F, device=dev, dtype=torch.bfloat16, generator=g) * 0.1
        cache = torch.zeros(F, ldc, device=dev, dtype=torch.bfloat16)[:, :M]
        sets.append((w.to(torch.bfloat16), w8, x, bias, cache, torch.empty(M, F, device=dev, dtype=torch.bfloat16)))
    sb = torch.full((F,) if rows else (1,), 1 / 512.0, device=dev)
    inds = rand_rows(G, F, keep, g)
    counts = torch.full((G,), keep, dtype=torch.int32, device=dev)
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % L
        return sets[state["i"]]

    def run_w8():
        _, w8, x, bias, cache, out = nxt()
        torch.ops.chipmunk.csp_mlp_mm1_w8(x, w8, sb, out, bias, cache, inds, counts, "gelu_tanh", True)

    def run_bf16():
        w16, _, x, bias, cache, out = nxt()
        torch.ops.chipmunk.csp_mlp_mm1_scatter(x, w16, out, bias, cache, inds, counts)
    rounds = int(os.environ.get("KB_ROUNDS", "5"))
    t = {"w8": [], "bf16": []}
    for _ in range(rounds):
        t["w8"].append(timeit(run_w8) * 1e3)
        t["bf16"].append(timeit(run_bf16) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    flops = 2.0 * M * K * keep
    tag = f"(M={M} K={K} F={F} keep={keep} layers={L} scales={'row' if rows else 'tensor'}, {rounds} alternating rounds)"
    print(f"mm1_w8  e4m3 rows: {med['w8']:8.1f} us  [{min(t['w8']):.1f} .. {max(t['w8']):.1f}]  {flops/med['w8']/1e6:7.1f} TFLOP/s   {tag}")
    print(f"mm1s    bf16 rows: {med['bf16']:8.1f} us  [{min(t['bf16']):.1f} .. {max(t['bf16']):.1f}]  {flops/med['bf16']/1e6:7.1f} TFLOP/s")
    print(f"mm1_w8 / mm1s    : {med['w8'] / med['bf16']:8.3f}")
    # the block-mean probe of a selecting step: [G, K] rows through fc1
    lin = torch.nn.Linear(K, F, device=dev, dtype=torch.bfloat16)
    q = W8Linear.from_linear(lin, scaling="row" if rows else "tensor")
    xm = torch.randn(1, G, K, device=dev, dtype=torch.bfloat16, generator=g)
    tp = {"w8": [], "bf16": []}
    with torch.no_grad():
        for _ in range(rounds):
            tp["w8"].append(timeit(lambda: q(xm)) * 1e3)
            tp["bf16"].append(timeit(lambda: lin(xm)) * 1e3)
    mp = {k: sorted(v)[len(v) // 2] for k, v in tp.items()}
    print(f"probe fc1(block_mean(x)) [{G} x {K}] -> {F}: W8Linear {mp['w8']:8.1f} us  [{min(tp['w8']):.1f} .. {max(tp['w8']):.1f}]   "
          f"nn.Linear {mp['bf16']:8.1f} us  [{min(tp['bf16']):.1f} .. {max(tp['bf16']):.1f}]   ratio {mp['w8'] / mp['bf16']:.2f}")


def bench_mm1_glu_w8(M=4352, K=3072, F=12288, keep=3840, act="silu"):
    """The gated weight-only fp8 GEMM1 (csp_mlp_mm1_glu_w8: e4m3 rows of the gate / up weights, bf16 activations) against the bf16
    csp_mlp_mm1_glu on the widened weights, at the FLUX gated shape of bench_mm1_glu, same activations and index lists.  Same process, the
    two alternating (KB_ROUNDS pairs, default 5); per launch the median bracket of `timeit` (20 launches, clocks warmed), then the median
    and the range over the rounds.  KB_LAYERS=n rotates n sets of weights / caches / outputs (n = 8: the weight rows come from HBM).
    KB_W8_SCALES=row: one scale per weight row instead of one number; KB_GLU_UPDATE=0 times the forms without the scatter-add."""
    g = torch.Generator(device=dev).manual_seed(0)
    L = int(os.environ.get("KB_LAYERS", "1"))
    rows = os.environ.get("KB_W8_SCALES", "tensor") == "row"
    upd = os.environ.get("KB_GLU_UPDATE", "1") == "1"
    G = (M + 127) // 128
    sets = []
    for _ in range(L):
        w = torch.randn(2 * F, K, device=dev, generator=g) * 0.02      # the halves of one fused projection
        w8 = (w * 512).clamp(-448, 448).to(torch.float8_e4m3fn)
        w16 = (w8.to(torch.bfloat16) * (1 / 512.0)).contiguous()      # the widened weight: exact
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, generator=g) * 0.5
        cache = torch.zeros(F, M, device=dev, dtype=torch.bfloat16)
        sets.append((w16, w8, x, cache, torch.empty(M, F, device=dev, dtype=torch.bfloat16)))
    sg, su = (torch.full((F,) if rows else (1,), 1 / 512.0, device=dev) for _ in range(2))
    inds = rand_rows(G, F, keep, g)
    counts = torch.full((G,), keep, dtype=torch.int32, device=dev)
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % L
        return sets[state["i"]]

    def run_w8():
        _, w8, x, cache, out = nxt()
        torch.ops.chipmunk.csp_mlp_mm1_glu_w8(x, w8[:F], w8[F:], sg, su, out, None, None, cache, inds, counts, act, upd)

    def run_bf16():
        w16, _, x, cache, out = nxt()
        torch.ops.chipmunk.csp_mlp_mm1_glu(x, w16[:F], w16[F:], out, None, None, cache, inds, counts, act, upd)
    rounds = int(os.environ.get("KB_ROUNDS", "5"))
    t = {"w8": [], "bf16": []}
    for _ in range(rounds):
        t["w8"].append(timeit(run_w8) * 1e3)
        t["bf16"].append(timeit(run_bf16) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    flops = 2.0 * M * K * 2 * keep
    tag = (f"(M={M} K={K} F={F} keep={keep} {act} layers={L} scales={'row' if rows else 'tensor'} {'scatter' if upd else 'update off'}, "
           f"{rounds} alternating rounds)")
    print(f"mm1_glu_w8 e4m3 rows: {med['w8']:8.1f} us  [{min(t['w8']):.1f} .. {max(t['w8']):.1f}]  {flops/med['w8']/1e6:7.1f} TFLOP/s   {tag}")
    print(f"mm1_glu    bf16 rows: {med['bf16']:8.1f} us  [{min(t['bf16']):.1f} .. {max(t['bf16']):.1f}]  {flops/med['bf16']/1e6:7.1f} TFLOP/s")
    print(f"mm1_glu_w8 / mm1_glu: {med['w8'] / med['bf16']:8.3f}")


def bench_w8_probe(M=34, K=3072, F=12288):
    """The few-row weight-only forward (ops.w8_linear: the e4m3 weight streamed once, widened in registers) against W8Linear.forward with
    mlp.w8_stream_rows off (the whole weight widened to bf16 per call, then F.linear) and the bf16 nn.Linear over the widened weight, on the
    same rows: the block-mean probe fc1(block_mean(x)) of a selecting sparse step.  Same process, the three alternating (KB_ROUNDS rounds,
    default 5); per launch the median bracket of `timeit`, then the median and the range over the rounds.  KB_LAYERS=n rotates n layers
    (weights, inputs) per launch (n = 8 at the FLUX shape: 0.3 GB of e4m3 and 0.6 GB of bf16 weights, beyond the Infinity Cache: cold
    weights); KB_W8_SCALES=row: one scale per output feature."""
    from chipmunk_amd import ops
    from chipmunk_amd.modules import W8Linear
    from chipmunk_amd.util.config import GLOBAL_CONFIG
    g = torch.Generator(device=dev).manual_seed(0)
    L = int(os.environ.get("KB_LAYERS", "1"))
    rows = os.environ.get("KB_W8_SCALES", "tensor") == "row"
    sets = []
    for _ in range(L):
        lin = torch.nn.Linear(K, F, device=dev, dtype=torch.bfloat16)
        q = W8Linear.from_linear(lin, scaling="row" if rows else "tensor")
        with torch.no_grad():
            lin.weight.copy_(q.widened())
        sets.append((q, lin, torch.randn(M, K, device=dev, dtype=torch.bfloat16, generator=g)))
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % L
        return sets[state["i"]]

    def run_kernel():
        q, _, x = nxt()
        ops.w8_linear(x, q.weight, q.scale_reciprocal, q.bias)

    def run_widened():
        q, _, x = nxt()
        q(x)

    def run_bf16():
        _, lin, x = nxt()
        lin(x)
    GLOBAL_CONFIG["mlp"]["w8_stream_rows"] = 0
    rounds = int(os.environ.get("KB_ROUNDS", "5"))
    t = {"kernel": [], "widened": [], "bf16": []}
    with torch.no_grad():
        for _ in range(rounds):
            t["kernel"].append(timeit(run_kernel) * 1e3)
            t["widened"].append(timeit(run_widened) * 1e3)
            t["bf16"].append(timeit(run_bf16) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    tag = f"(M={M} K={K} F={F} layers={L} scales={'row' if rows else 'tensor'}, {rounds} alternating rounds)"
    print(f"w8_probe  w8_linear kernel : {med['kernel']:8.1f} us  [{min(t['kernel']):.1f} .. {max(t['kernel']):.1f}]  "
          f"{F * K / med['kernel'] / 1e6:6.2f} TB/s on the weight stream   {tag}")
    print(f"w8_probe  W8Linear widened : {med['widened']:8.1f} us  [{min(t['widened']):.1f} .. {max(t['widened']):.1f}]")
    print(f"w8_probe  bf16 nn.Linear   : {med['bf16']:8.1f} us  [{min(t['bf16']):.1f} .. {max(t['bf16']):.1f}]")
    print(f"w8_probe  kernel / widened : {med['kernel'] / med['widened']:8.3f}    kernel / nn.Linear: {med['kernel'] / med['bf16']:8.3f}")


def bench_fp8_wan(M=32768, ldc=None):
    """BASELINE config C5 (Wan2.1-1.3B, 832x480x81 -> 32 760 tokens padded to 32 768): fp8 e4m3 GEMM1, M = 32768, K = 1536,
    F = 8960, keep 0.3 (2688 columns); bf16 GEMM1 at the same shape beside it.  M = 32760: the ragged launch on the tokens as they are
    (ldc: the cache as the [:, :M] view of a [F, ldc] buffer, default the contiguous [F, M])."""
    g = torch.Generator(device=dev).manual_seed(0)
    K, F, keep = 1536, 8960, 2688
    B, loop = batch_env()     # KB_BATCH / KB_BATCH_LOOP as in bench_mlp
    a = torch.randn(B, M, K, device=dev, generator=g)
    w = torch.randn(F, K, device=dev, generator=g) * 0.02
    a8, w8 = (a * 16).clamp(-448, 448).to(torch.float8_e4m3fn), (w * 512).clamp(-448, 448).to(torch.float8_e4m3fn)
    sa, sb = torch.tensor([1 / 16.0], device=dev), torch.tensor([1 / 512.0], device=dev)
    bias = torch.zeros(F, device=dev, dtype=torch.bfloat16)
    cache = torch.randn(B, F, ldc or M, device=dev, dtype=torch.bfloat16, generator=g)[..., :M]
    packed = torch.empty(B, M, F, device=dev, dtype=torch.bfloat16)
    G = (M + 127) // 128
    inds = rand_rows(B * G, F, keep, g).view(B, G, F)
    counts = torch.full((B, G), keep, dtype=torch.int32, device=dev)
    flops = 2.0 * B * M * K * keep
    sel = list(range(B)) if loop or B == 1 else [slice(None)]     # the operands of every launch of one call

    def run_fp8():
        for b in sel:
            torch.ops.chipmunk.csp_mlp_mm1_fp8(a8[b], w8, packed[b], bias, cache[b], inds[b], counts[b], sa, sb, False)
    ms = timeit(run_fp8, reps=5)
    print(f"mm1_fp8 (Wan C5): {ms*1e3:8.1f} us  {flops/ms/1e9:7.1f} TFLOP/s   (M={M} K={K} F={F} keep={keep} ldc={ldc or M}{batch_tag(B, loop)})")
    ab, wb = a.to(torch.bfloat16), w.to(torch.bfloat16)

    def run_bf16():
        for b in sel:
            torch.ops.chipmunk.csp_mlp_mm1(ab[b], wb, packed[b], bias, cache[b], inds[b], counts[b])
    ms = timeit(run_bf16, reps=5)
    print(f"mm1 bf16 same shape: {ms*1e3:8.1f} us  {flops/ms/1e9:7.1f} TFLOP/s")


def bench_fp8_rs_wan(M=32768, act="silu"):
    """fp8 row scales at the Wan fp8 shape (M = 32768, K = 1536, F = 8960, keep 0.3): csp_mlp_mm1_fp8_act_rs (scale vectors [M] / [F])
    against csp_mlp_mm1_fp8_act (two numbers) on the same operands, alternating; then the row-wise input quantiser against the torch
    chain it replaces and against the per-tensor quantize_fp8, in us and GB/s of the 3 * rows * K + 4 * rows bytes it has to move."""
    g = torch.Generator(device=dev).manual_seed(0)
    K, F, keep = 1536, 8960, 2688
    a = torch.randn(M, K, device=dev, generator=g)
    w = torch.randn(F, K, device=dev, generator=g) * 0.02
    a8, w8 = (a * 16).clamp(-448, 448).to(torch.float8_e4m3fn), (w * 512).clamp(-448, 448).to(torch.float8_e4m3fn)
    sa, sb = torch.tensor([1 / 16.0], device=dev), torch.tensor([1 / 512.0], device=dev)
    sav, sbv = sa.expand(M).contiguous(), sb.expand(F).contiguous()
    bias = torch.zeros(F, device=dev, dtype=torch.bfloat16)
    cache = torch.randn(F, M, device=dev, dtype=torch.bfloat16, generator=g)
    packed = torch.empty(M, F, device=dev, dtype=torch.bfloat16)
    G = (M + 127) // 128
    inds = rand_rows(G, F, keep, g)
    counts = torch.full((G,), keep, dtype=torch.int32, device=dev)
    flops = 2.0 * M * K * keep
    runs = {"scalar": lambda: torch.ops.chipmunk.csp_mlp_mm1_fp8_act(a8, w8, packed, bias, cache, inds, counts, sa, sb, act, 0),
            "vectors": lambda: torch.ops.chipmunk.csp_mlp_mm1_fp8_act_rs(a8, w8, packed, bias, cache, inds, counts, sav, sbv, act, 0)}
    t = {k: [] for k in runs}
    for _ in range(5):      # alternating, so that a drift of the box falls on both
        for k, fn in runs.items():
            t[k].append(timeit(fn, reps=5) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    for k in runs:
        print(f"mm1_fp8_act {k:8s} {act}: {med[k]:8.1f} us  [{min(t[k]):.1f} .. {max(t[k]):.1f}]  {flops/med[k]/1e6:7.1f} TFLOP/s   (M={M} K={K} F={F} keep={keep})")
    print(f"vectors / scalar: {med['vectors'] / med['scalar']:7.3f}")
    x = a.to(torch.bfloat16)
    scale = torch.tensor(16.0, device=dev)

    def chain():
        xf = x.float()
        s = (torch.full((M,), 448.0, device=dev) / xf.abs().amax(dim=-1).clamp(min=1e-12)).clamp(max=448.0)
        return (xf * s[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn), s.reciprocal()
    qs = {"quantize_fp8_rowwise": lambda: torch.ops.chipmunk.quantize_fp8_rowwise(x, 448.0), "torch row chain": chain,
          "quantize_fp8 (per tensor)": lambda: torch.ops.chipmunk.quantize_fp8(x, scale.reshape(1), 448.0)}
    bytes_moved = 3.0 * M * K + 4.0 * M
    for k, fn in qs.items():
        us = sorted(timeit(fn, reps=10) * 1e3 for _ in range(3))
        print(f"{k:26s}: {us[1]:8.1f} us  [{us[0]:.1f} .. {us[2]:.1f}]  {bytes_moved / us[1] / 1e3:7.1f} GB/s of 3 * rows * K + 4 * rows bytes   (rows={M} K={K})")


def bench_cache_groups(which, M, K, F, keep, fp8):
    """The two layouts of the activation cache under one GEMM1 (mlp.cache_layout; DESIGN 4.2, "Group-major cache"): the column-major
    [F, M] against the group-major [ceil(M/128), F, 128] holding the same values, same operator (csp_mlp_mm1_fp8_act with the scatter-add
    of its deltas at the Wan fp8 shape, csp_mlp_mm1_act with it at the FLUX bf16 shape), same operands, alternating in one process
    (KB_ROUNDS pairs, default 5); median and range over the rounds of `timeit`'s median bracket.  KB_LAYERS=n rotates n sets of weights /
    caches / outputs (n = 30: the loop's cold-cache condition, every layer's cache pieces come from HBM)."""
    g = torch.Generator(device=dev).manual_seed(0)
    L = int(os.environ.get("KB_LAYERS", "1"))
    G = (M + 127) // 128
    a = torch.randn(M, K, device=dev, generator=g)
    a = (a * 16).clamp(-448, 448).to(torch.float8_e4m3fn) if fp8 else a.to(torch.bfloat16)
    sa, sb = torch.tensor([1 / 16.0], device=dev), torch.tensor([1 / 512.0], device=dev)
    bias = torch.zeros(F, device=dev, dtype=torch.bfloat16)
    packed = torch.empty(M, F, device=dev, dtype=torch.bfloat16)
    inds = rand_rows(G, F, keep, g)
    counts = torch.full((G,), keep, dtype=torch.int32, device=dev)
    sets = []
    for _ in range(L):
        w = torch.randn(F, K, device=dev, generator=g) * 0.02
        w = (w * 512).clamp(-448, 448).to(torch.float8_e4m3fn) if fp8 else w.to(torch.bfloat16)
        col = torch.randn(F, M, device=dev, dtype=torch.bfloat16, generator=g) * 0.1
        grp = torch.nn.functional.pad(col, (0, G * 128 - M)).view(F, G, 128).permute(1, 0, 2).contiguous()
        sets.append((w, col, grp))
    state = {"i": 0}

    def run(layout):
        state["i"] = (state["i"] + 1) % L
        w, col, grp = sets[state["i"]]
        cache = grp if layout == "group" else col
        if fp8:
            torch.ops.chipmunk.csp_mlp_mm1_fp8_act(a, w, packed, bias, cache, inds, counts, sa, sb, "gelu_tanh", 2)
        else:
            torch.ops.chipmunk.csp_mlp_mm1_act(a, w, packed, bias, cache, inds, counts, "gelu_tanh", True)
    rounds = int(os.environ.get("KB_ROUNDS", "5"))
    t = {"column": [], "group": []}
    for _ in range(rounds):      # alternating, so that a drift of the box falls on both
        for k in t:
            t[k].append(timeit(lambda: run(k), reps=5 if M > 8192 else 20) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    flops = 2.0 * M * K * keep
    tag = f"(M={M} K={K} F={F} keep={keep} layers={L}, {rounds} alternating rounds)"
    for k in t:
        print(f"{which} cache {k:6s}: {med[k]:8.1f} us  [{min(t[k]):.1f} .. {max(t[k]):.1f}]  {flops/med[k]/1e6:7.1f} TFLOP/s   {tag}")
    print(f"{which} group / column: {med['group'] / med['column']:7.3f}")


def bench_to_groups(R, C, B=1):
    """transpose_to_groups ([B, R, C] -> [B, ceil(R/128), C, 128], the full step's cache of mlp.cache_layout: group) against transpose_last2
    ([B, C, R]) on the same activations, alternating; us and GB/s of the 4 * B * R * C bytes both have to move."""
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, R, C, device=dev, dtype=torch.bfloat16, generator=g)
    runs = {"transpose_last2": lambda: torch.ops.chipmunk.transpose_last2(x), "transpose_to_groups": lambda: torch.ops.chipmunk.transpose_to_groups(x)}
    t = {k: [] for k in runs}
    for _ in range(int(os.environ.get("KB_ROUNDS", "5"))):
        for k, fn in runs.items():
            t[k].append(timeit(fn, reps=10) * 1e3)
    for k, v in t.items():
        med = sorted(v)[len(v) // 2]
        print(f"{k:20s}: {med:8.1f} us  [{min(v):.1f} .. {max(v):.1f}]  {4.0 * B * R * C / med / 1e3:7.1f} GB/s   (B={B} R={R} C={C})")


def sorted_random_indices(H, G, n_keys, count, width, g):
    inds = torch.zeros(1, H, G, width, dtype=torch.int32, device=dev)
    for h in range(H):
        r = torch.rand(G, n_keys, device=dev, generator=g)
        inds[0, h, :, :count] = r.topk(count, dim=-1).indices.sort(dim=-1).values.to(torch.int32)
    return inds


def bench_attn(which, variants):
    g = torch.Generator(device=dev).manual_seed(0)
    if "hunyuan" in which:
        H, N, count = int(os.environ.get('KB_HEADS', '6')), int(os.environ.get('KB_N', '119056')), int(os.environ.get('KB_COUNT_C3', '7296'))   # BASELINE C3 counts; KB_HEADS=24 for all heads
    else:
        H, N, count = 24, 4352, int(os.environ.get('KB_COUNT', '672'))
    q, k, v = [torch.randn(1, H, N, 128, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(3)]
    G = (N + 191) // 192
    for var in variants:
        _native.set_option("attn_variant", var)
        if which.startswith("csp"):
            inds = sorted_random_indices(H, G, N, count, N, g)
            if os.environ.get("KB_SAME_INDICES") == "1":   # every query group of a head gathers the same keys: all gathers hit L2
                inds[:] = inds[:, :, :1].clone()
            counts = torch.full((1, H, G), count, dtype=torch.int32, device=dev)
            o = torch.zeros_like(q)
            ms = timeit(lambda: torch.ops.chipmunk.csp_attn(q, k, v, o, inds, counts, 1), reps=10)
            flops = 98304.0 * count * H * G
            del inds
        elif which.startswith("dense"):
            ms = timeit(lambda: torch.ops.chipmunk.dense_attn(q, k, v), reps=5)
            flops = 4.0 * H * N * N * 128
        elif which.startswith("colsum"):
            _, l = torch.ops.chipmunk.dense_attn(q, k, v)
            ms = timeit(lambda: torch.ops.chipmunk.dense_colsum_attn(q, k, v, l), reps=5)
            flops = 4.0 * H * N * N * 128
        elif which.startswith("maskstep"):
            # the mask-recompute step's attention: dense + column sums + top-k mask in one op (7 % of the keys kept)
            _, l = torch.ops.chipmunk.dense_attn(q, k, v)
            ktop = int(os.environ.get("KB_KTOP", str(int(0.07 * N))))
            ms = timeit(lambda: torch.ops.chipmunk.dense_colsum_topk_mask(q, k, v, l, ktop, 0.0, None, None, False), reps=5)
            flops = 4.0 * H * N * N * 128
        elif which.startswith("sdpa"):
            ms = timeit(lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v), reps=5)
            flops = 4.0 * H * N * N * 128
        print(f"{which:12s} variant {var}: {ms*1e3:9.1f} us  {flops/ms/1e9:7.1f} TFLOP/s   (H={H} N={N} count={count})")
    _native.set_option("attn_variant", 0)


def bench_io(which):
    g = torch.Generator(device=dev).manual_seed(0)
    if which == "topk":
        act = torch.randn(1, 34, 12288, device=dev, generator=g).abs().to(torch.bfloat16)
        inds = torch.empty(1, 34, 12288, dtype=torch.int32, device=dev)
        counts = torch.empty(1, 34, dtype=torch.int32, device=dev)
        ms = timeit(lambda: torch.ops.chipmunk.topk_indices(act, inds, counts, 0.7, 256, 0.05))
        print(f"topk_indices [1,34,12288]: {ms*1e3:8.1f} us")
    elif which == "topkd":
        # the fused |b - cache| -> top-k -> copy kernel of the sparse MLP step, KB_LAYERS sets of (b, cache) rotating
        L = int(os.environ.get("KB_LAYERS", "1"))
        sets = []
        for _ in range(L):
            b = torch.randn(1, 34, 12288, device=dev, generator=g).to(torch.bfloat16)
            c = (b.float() + 0.3 * torch.randn(1, 34, 12288, device=dev, generator=g)).to(torch.bfloat16)
            sets.append((b, c, torch.empty(1, 34, 12288, dtype=torch.int32, device=dev),
                         torch.empty(1, 34, dtype=torch.int32, device=dev)))
        # evict between launches like the real loop does: a 300 MB memset-sized touch is too slow; rotate instead
        st = {"i": 0}

        def run():
            st["i"] = (st["i"] + 1) % L
            b, c, inds, counts = sets[st["i"]]
            torch.ops.chipmunk.topk_delta_indices(b, c, inds, counts, 0.7, 256, 0.05)
        ms = timeit(run)
        print(f"topk_delta_indices [1,34,12288] layers={L}: {ms*1e3:8.1f} us")
    elif which == "m2i":
        H, G, N = 24, 621, 119232
        mask = torch.rand(1, H, G, N, device=dev, generator=g) < 0.06
        ms = timeit(lambda: torch.ops.chipmunk.mask_to_indices(mask, 128, 192), reps=5)
        byts = H * G * N + 4 * 0.06 * H * G * N
        print(f"mask_to_indices [1,24,621,119232]: {ms*1e3:8.1f} us  {byts/ms/1e6:7.1f} GB/s algorithmic")
        packed, shp = chipmunk_amd.ops.bitpack(mask)
        ms = timeit(lambda: chipmunk_amd.ops.packed_mask_to_indices(packed, shp, 128, 192), reps=5)
        byts = H * G * N / 8 + 4 * 0.06 * H * G * N
        print(f"packed_mask_to_indices           : {ms*1e3:8.1f} us  {byts/ms/1e6:7.1f} GB/s algorithmic")
        ms = timeit(lambda: chipmunk_amd.ops.mask_to_sorted_indices(packed, shp, 128, 192), reps=5)
        print(f"packed mask -> sorted indices    : {ms*1e3:8.1f} us  {byts/ms/1e6:7.1f} GB/s algorithmic")
        ms = timeit(lambda: chipmunk_amd.ops.bitunpack(packed, shp), reps=5)
        print(f"bitunpack                        : {ms*1e3:8.1f} us  {(H*G*N*1.125)/ms/1e6:7.1f} GB/s")
        ms = timeit(lambda: chipmunk_amd.ops.bitpack(mask), reps=5)
        print(f"bitpack                          : {ms*1e3:8.1f} us  {(H*G*N*1.125)/ms/1e6:7.1f} GB/s")
    elif which == "copy":
        src = torch.randn(1, 34, 12288, device=dev).to(torch.bfloat16)
        dst = torch.zeros_like(src)
        inds = torch.stack([torch.randperm(12288, device=dev) for _ in range(34)]).to(torch.int32)[None]
        counts = torch.full((1, 34), 4096, dtype=torch.int32, device=dev)
        ms = timeit(lambda: torch.ops.chipmunk.copy_indices(src, dst, inds, counts))
        print(f"copy_indices [1,34,12288] keep 4096: {ms*1e3:8.1f} us")


def bench_group_delta():
    """The selection of a sparse MLP step whose groups own R block-mean rows: the modules' torch chain (sub, abs, reshape + sum, two
    empties, topk_indices, copy_indices -- temporaries included) against topk_group_delta_indices, same box, both orders.
    Cold rows: every launch of a bracket takes another (activation, cache) set, enough sets for ~1 GB in all (the LLC holds 256 MB), and
    the caches are put back before every bracket, outside it, in the order the bracket visits them -- the copy makes the listed columns
    of the cache equal the activations, so a second launch on the same set would rank another row of scores.
    KB_ROUNDS brackets per side and order (default 5); the figure is the median, with the range."""
    ops = chipmunk_amd.ops
    rounds = int(os.environ.get("KB_ROUNDS", "5"))
    g = torch.Generator(device=dev).manual_seed(0)
    #        name                                rows      F      R
    shapes = [("Wan-sized gated", 2 * 256, 8960, 2), ("FLUX-sized gated", 2 * 36, 12288, 2), ("HunyuanVideo-sized gated", 2 * 930, 13824, 2),
              ("Wan-sized ungated, bm = 4 mbm", 2 * 256, 8960, 4)]
    for name, rows, F, R in shapes:
        G = rows // R
        set_bytes = 2 * rows * F * 2 + G * F * 4
        L = min(256, max(16, -(-(1 << 30) // set_bytes)))
        sets = []
        for _ in range(L):
            b = torch.randn(1, rows, F, device=dev, generator=g).to(torch.bfloat16)
            c0 = (b.float() + 0.3 * torch.randn(1, rows, F, device=dev, generator=g)).to(torch.bfloat16)
            sets.append((b, c0, c0.clone()))
        inds_f = [torch.empty(1, G, F, dtype=torch.int32, device=dev) for _ in range(L)]
        counts_f = torch.empty(1, G, dtype=torch.int32, device=dev)

        def unfused(b, cache):
            mdiff = (b - cache).abs()
            bsz, _rows, f = mdiff.shape
            mdiff = mdiff.reshape(bsz, -1, R, f).sum(dim=2)
            inds = torch.empty_like(mdiff, dtype=torch.int32, device=dev)
            counts = torch.empty((mdiff.size(0), mdiff.size(1)), dtype=torch.int32, device=dev)
            ops.topk_indices(mdiff, inds, counts, 0.7, 256, 0.0)
            ops.copy_indices(b, cache, inds, counts)
            return inds, counts

        def fused(b, cache, i):
            ops.topk_group_delta_indices(b, cache, inds_f[i], counts_f, R, 0.7, 256, 0.0)

        def bracket(side):
            for b, c0, c in sets:
                c.copy_(c0)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i, (b, _c0, c) in enumerate(sets):
                unfused(b, c) if side == "unfused" else fused(b, c, i)
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / L * 1e3      # us per selection

        warm_gpu()
        # same results at the timed size (R == 2: bit for bit; R > 2: torch's reduction order is not the contract -- reported, not asserted)
        b, c0, c = sets[0]
        ui, uc = unfused(b, c)
        ucache = c.clone()
        c.copy_(c0)
        fused(b, c, 0)
        torch.cuda.synchronize()
        listed = torch.arange(F, device=dev) < uc[..., None]
        same = (torch.equal(uc, counts_f) and torch.equal(torch.where(listed, ui, -1), torch.where(listed, inds_f[0], -1))
                and torch.equal(ucache.view(torch.int16), c.view(torch.int16)))
        for side in ("unfused", "fused"):      # every shape once before anything is timed
            bracket(side)
        res = {"unfused first": {"unfused": [], "fused": []}, "fused first": {"unfused": [], "fused": []}}
        for _ in range(rounds):
            for order in ("unfused first", "fused first"):
                for side in (("unfused", "fused") if order == "unfused first" else ("fused", "unfused")):
                    res[order][side].append(bracket(side))
        print(f"group_delta {name} [1,{rows},{F}] R={R} G={G} sets={L} rounds={rounds} same_result={same}")
        for order, sides in res.items():
            for side, v in sides.items():
                v = sorted(v)
                print(f"  {order:13s} {side:8s} median {v[len(v) // 2]:8.1f} us  range {v[0]:8.1f} .. {v[-1]:8.1f}")
        del sets, inds_f
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["mm1", "mm2", "scatter", "csp_flux", "dense_flux", "sdpa_flux", "topk"])
    ap.add_argument("--variants", default="0")
    ap.add_argument("--opt", action="append", default=[], help="name=value tuning option (repeatable)")
    args = ap.parse_args()
    for o in args.opt:
        name, val = o.split("=")
        _native.set_option(name, int(val))
    variants = [int(x) for x in args.variants.split(",")]
    for w in args.what:
        if w in ("mm1", "mm1s", "mm2", "scatter"):
            bench_mlp(w, variants, keep=int(os.environ.get("KB_KEEP", "4096")))   # KB_KEEP: kept columns per group (FLUX: 0.3 * 12288 -> 3840)
        elif w == "mm1_glu":          # gated GEMM1 at the FLUX MLP shape against the ungated launch of equal work (KB_GLU_ACT: silu, gelu_tanh, gelu)
            bench_mm1_glu(act=os.environ.get("KB_GLU_ACT", "silu"))
        elif w == "mm1_act":          # ungated GEMM1 with SiLU / exact GELU / tanh-GELU at the FLUX MLP shape against csp_mlp_mm1_scatter
            bench_mm1_act()
        elif w == "mm1_glu_fp8":      # gated fp8 GEMM1 at the Wan fp8 shape against the ungated fp8 launch of equal work (KB_GLU_ACT as mm1_glu)
            bench_mm1_glu_fp8(act=os.environ.get("KB_GLU_ACT", "silu"))
        elif w == "mm2_w8":           # weight-only fp8 GEMM2 against the bf16 GEMM2 at the FLUX shape, 30 % of 12 288 columns kept
            bench_mm2_w8()
        elif w == "mm1_w8":           # weight-only fp8 GEMM1 (+ scatter-add) against mm1s at the FLUX shape, 3 840 of 12 288 columns kept
            bench_mm1_w8()
        elif w == "mm1_w8_wan":       # ... at the Wan2.1 1.3B shape: 32 760 tokens (ragged last group), K = 1 536, F = 8 960, 2 816 kept
            bench_mm1_w8(M=32760, K=1536, F=8960, keep=2816)
        elif w == "mm1_glu_w8":       # gated weight-only fp8 GEMM1 against the bf16 gated GEMM1 on the widened weights, FLUX gated shape (KB_GLU_ACT)
            bench_mm1_glu_w8(act=os.environ.get("KB_GLU_ACT", "silu"))
        elif w == "w8_probe":         # few-row weight-only forward at the FLUX probe shape [34, 3072] -> 12288: kernel / widened W8Linear / nn.Linear
            bench_w8_probe()
        elif w == "w8_probe_wan":     # ... at the Wan2.1 1.3B probe shape [256, 1536] -> 8960
            bench_w8_probe(M=256, K=1536, F=8960)
        elif w == "w8_probe_hunyuan": # ... at the HunyuanVideo probe shape [931, 3072] -> 12288
            bench_w8_probe(M=931, K=3072, F=12288)
        elif w == "mm2_w8_wan":       # ... at the Wan2.1 1.3B shape: 32 760 tokens (ragged last group), N2 = 1 536, F = 8 960, 2 816 kept
            bench_mm2_w8(M=32760, F=8960, N2=1536, keep=2816)
        elif w == "fp8_wan":
            bench_fp8_wan()
        elif w == "fp8_rs_wan":       # fp8 GEMM1 with scale vectors against the scalar launch, and the row-wise input quantiser (KB_GLU_ACT as mm1_glu)
            bench_fp8_rs_wan(act=os.environ.get("KB_GLU_ACT", "silu"))
        elif w == "fp8_wan_groups":   # fp8 GEMM1 + scatter-add at the Wan shape: column-major against group-major cache (KB_LAYERS, KB_ROUNDS)
            bench_cache_groups("mm1_fp8 (Wan C5)", M=32768, K=1536, F=8960, keep=2688, fp8=True)
        elif w == "mm1s_groups":      # bf16 GEMM1 + scatter-add at the FLUX shape: column-major against group-major cache
            bench_cache_groups("mm1s (FLUX)", M=4352, K=3072, F=12288, keep=int(os.environ.get("KB_KEEP", "3840")), fp8=False)
        elif w == "to_groups":        # the full step's layout kernel against transpose_last2 at the Wan and HunyuanVideo activation shapes
            bench_to_groups(32760, 8960)
            bench_to_groups(119056, 12288)
        elif w == "mm2_wan":          # GEMM2 at the Wan2.1 1.3B shape (configs[4]): M = 32 768 rows, N2 = 1 536, F = 8 960, 30 % kept
            bench_mlp("mm2", variants, M=32768, K=1536, F=8960, keep=2816)
        elif w == "fp8_wan_ragged":   # the same launches on Wan2.1's 32 760 tokens as they are: 255 groups + 120 rows
            bench_fp8_wan(M=32760)
        elif w == "fp8_wan_ragged_pitched":   # ... with the cache columns on 128-byte lines (ldc = 32 768)
            bench_fp8_wan(M=32760, ldc=32768)
        elif w == "mm2_wan_ragged":
            bench_mlp("mm2", variants, M=32760, K=1536, F=8960, keep=2816)
        elif w in ("mm1s_hunyuan", "mm2_hunyuan"):   # HunyuanVideo 720x1280x129: 119 056 tokens = 930 groups + 16 rows, 30 % of 12 288 columns kept
            bench_mlp(w.split("_")[0], variants, M=119056, K=3072, F=12288, keep=3840)
        elif w in ("topk", "topkd", "m2i", "copy"):
            bench_io(w)
        elif w == "group_delta":      # selection over R block-mean rows per group: the modules' torch chain against the fused operator
            bench_group_delta()
        else:
            bench_attn(w, variants)


if __name__ == "__main__":
    main()
