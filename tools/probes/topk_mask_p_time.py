"""Launch times of the mask selection at the C3 row (n = 119 056, KB_ROWS rows, default 24 * 621), the figures of DESIGN.md 4.3:
chipmunk_topk_mask from this tree's library and from a second build of the library (KB_OTHER_LIB = path of a libchipmunk_hip.so,
e.g. built from the parent commit; default: this tree's again), the two alternating, register and streaming form; then
chipmunk_topk_mask_p in both forms at top_p 0.9 / 0.95 / 0.99 with the kept keys per row.  C ABI through ctypes on the null stream,
device events.  Rows are SYNTHETIC: bf16(192 * softmax(3 * randn)) (KB_KIND = softmax) or |randn|."""
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
parent = ctypes.CDLL(os.environ["KB_OTHER_LIB"]) if os.environ.get("KB_OTHER_LIB") else branch
n, rows = 119056, int(os.environ.get("KB_ROWS", 24 * 621))
k = 128 * round(0.05 * n / 128)
g = torch.Generator(device=dev).manual_seed(3)
kind = os.environ.get("KB_KIND", "softmax")
if kind == "softmax":   # synthetic peaked rows: 192 * softmax(3 * randn), as the random rows of the tests
    cs = torch.empty(rows, n, dtype=torch.bfloat16, device=dev)
    for a in range(0, rows, 512):
        x = torch.randn(min(512, rows - a), n, device=dev, generator=g)
        cs[a:a + 512] = (192.0 * torch.softmax(3.0 * x, dim=-1)).to(torch.bfloat16)
else:
    cs = torch.randn(rows, n, device=dev, generator=g).abs().to(torch.bfloat16)
mask = torch.empty(rows, n, dtype=torch.bool, device=dev)
vp = ctypes.c_void_p


def plain(lib):
    rc = lib.chipmunk_topk_mask(vp(cs.data_ptr()), ctypes.c_int64(n), vp(0), ctypes.c_int64(0), 1, vp(0), vp(mask.data_ptr()), rows, n, k,
                                ctypes.c_double(0.01), vp(0))
    assert rc == 0, rc


def mass(top_p):
    rc = branch.chipmunk_topk_mask_p(vp(cs.data_ptr()), ctypes.c_int64(n), vp(0), ctypes.c_int64(0), 1, vp(0), vp(mask.data_ptr()), rows, n, k,
                                     ctypes.c_double(0.01), ctypes.c_double(top_p), 0, vp(0))
    assert rc == 0, rc


def t(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


out = {"n": n, "rows": rows, "k": k, "kind": kind}
for stream in (0, 1):
    for lib in (branch, parent):
        assert lib.chipmunk_set_option(b"topk_mask_stream", stream) == 0
    form = "stream" if stream else "register"
    a, b = [], []
    for _ in range(4):          # alternate the two builds: the spread of each is the box's run-to-run spread
        a.append(t(lambda: plain(branch)))
        b.append(t(lambda: plain(parent)))
    out[f"topk_mask {form} this tree ms"] = a
    out[f"topk_mask {form} other build ms"] = b
    for top_p in (0.9, 0.95, 0.99):
        out[f"topk_mask_p {form} top_p {top_p} ms"] = [t(lambda: mass(top_p)) for _ in range(2)]
        kept = mask.sum(-1).float()
        out[f"kept keys top_p {top_p} {form} (mean, min, max)"] = [float(kept.mean()), float(kept.min()), float(kept.max())]
    for lib in (branch, parent):
        lib.chipmunk_set_option(b"topk_mask_stream", 0)
for key, val in out.items():
    print(key, val)
if os.environ.get("KB_JSON"):
    with open(os.environ["KB_JSON"], "w") as f:
        json.dump(out, f, indent=1)
