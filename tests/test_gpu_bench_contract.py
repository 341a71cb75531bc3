"""bench.py's output contract on the GPU box, at reduced layer counts so the three workloads finish in well under a minute
each: ONE JSON line with the driver's keys; with --full a `roofline` object for the dominant kernel (HIP-event durations from the
timed region), a `cpu_baseline` object and the measured legs of the HunyuanVideo line; the sharded code paths at world size 1; a
plain run that measures the headline only and dumps the last timed step's outputs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
        "config", "roofline", "cpu_baseline"}


def _bench(*args, timeout=600, **extra_env):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f"stdout must carry exactly one line, got {len(lines)}"
    return json.loads(lines[0])


def _check_common(d, steps, warmup):
    assert KEYS <= set(d), KEYS - set(d)
    assert d["metric"] == "DiT denoise steps/sec at fixed sparsity" and d["unit"] == "steps/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and 0.02 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["launches_in_timed_region"] > 0 and r["avg_launch_ms"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert "workload" in d["config"] and "model" not in d["config"]


def test_hunyuan_line_with_its_legs():
    d = _bench("--full", "--layers", "4", "--steps", "3", "--warmup", "3")
    _check_common(d, 3, 3)
    assert d["config"]["workload"].startswith("hunyuan_c3") and d["dtype"] == "bf16" and d["scaling"] == "strong"
    assert set(d["kernels"]) >= {"dense_attn", "csp_128_attn"}
    comp = d["dense_gpu_comparator"]
    assert comp["sparse_over_dense"] > 1.0 and "FLASH" in comp["backend"] and comp["own_dense"]["sparse_over_own_dense"] > 1.0
    # the default run executes the shipped skip schedule in its timed region (BASELINE configs[2] "+ step caching") and reports what
    # unchanged model code (no fused row-wise operator) and norm-spread q / k would see
    assert d["config"]["step_caching"] is True and "step_caching_leg" not in d
    assert d["no_fused_rowwise_leg"]["sparse_step_s"] > 0 and d["no_fused_rowwise_leg"]["timed_region_steps_per_s_equivalent"] > 0
    assert 0.0 <= d["qk_norm_gain_leg"]["waves_on_the_loop_without_reference_point"] <= 1.0 and d["qk_norm_gain_leg"]["csp_128_attn_avg_ms"] > 0
    assert "aotriton" in d["sdpa_flash_libraries"] and "ck" in d["sdpa_flash_libraries"] and d["big_scratch_fallbacks"] == 0
    assert d["running_max_fallback_leg"]["csp_128_attn_avg_ms"] > 0
    assert 0.75 < d["sparsity_82_leg"]["column_sparsity"] < 0.86 and 0.90 < d["column_sparsity"] < 0.95
    assert d["roofline"]["traffic_source"] is None or d["roofline"]["traffic_source"].startswith("profiles/")
    # a 3-step window is not the schedule: the line says what the whole 50-step schedule runs at and how far the window is from it
    sys.path.insert(0, ROOT)
    import bench
    bench.check_window_declared(d)
    assert d["whole_schedule_steps_per_s"] > 0 and d["window_bias"] == pytest.approx(d["value"] / d["whole_schedule_steps_per_s"])
    assert d["tracking"]["every_step_computed_steps_5_24_steps_per_s"] > 0


def test_hunyuan_line_without_the_step_cache_has_the_step_caching_leg():
    d = _bench("--full", "--layers", "4", "--steps", "3", "--warmup", "3", "--no-step-caching", "--no-82", "--dense-steps", "0", "--no-cpu-baseline")
    assert d["config"]["step_caching"] is False
    leg = d["step_caching_leg"]
    assert leg["skipped"] == 6 and leg["kinds"].count("sparse") == 3 and leg["steps_per_s"] > d["value"]


@pytest.mark.parametrize("mode,chunks", [("heads", "8,16"), ("groups", "6,18")])
def test_sharded_paths_at_world_size_one(mode, chunks):
    d = _bench("--workload", "hunyuan_sp", "--sp-mode", mode, "--sp-chunks", chunks, "--layers", "3", "--steps", "2", "--warmup", "3",
               "--no-cpu-baseline", "--no-legs")
    assert d["config"]["sp_mode"] == mode and d["config"]["dist_world_size"] == 1 and d["scaling"] == "strong" and d["value"] > 0
    assert str([int(c) for c in chunks.split(",")]) in d["config"]["parallelism"]


def test_wan_and_flux_lines():
    w = _bench("--full", "--workload", "wan_c5", "--layers", "4", "--steps", "3", "--warmup", "12", "--dense-steps", "1")
    _check_common(w, 3, 12)
    assert w["config"]["workload"].startswith("wan_c5") and "fp8" in w["dtype"] and "csp_mlp_mm1_fp8" in w["kernels"]
    assert w["offload"]["modules_offloaded"] >= 1 and w["offload"]["pinned_host_bytes_read_per_sparse_step"] > 0
    assert w["invocation_kinds_seen"]["sparse"] > 0 and w["dense_gpu_comparator"]["sparse_over_dense"] > 0
    assert w["resident_leg"]["value"] > 0 and w["resident_leg"]["over_the_offloaded_run"] > 0.5   # the residency policy, measured by a second process
    f = _bench("--full", "--workload", "flux_c2", "--layers", "6", "--steps", "6", "--warmup", "12", "--dense-steps", "1")
    _check_common(f, 6, 12)
    assert f["config"]["workload"].startswith("flux_c2") and {"csp_attn", "csp_mlp_mm2"} <= set(f["kernels"])
    # microsecond-scale launches: only every 7th call of a timed op carries a HIP-event bracket (a bracket's bubble is ~10 us); all calls are counted
    for line in (w, f):
        assert line["event_brackets"]["every_nth_call_of_a_timed_op"] == 7
        for k in line["kernels"].values():
            assert 1 <= k["timed_launches"] <= k["launches"] and k["timed_launches"] <= k["launches"] // 7 + 1 and k["avg_ms"] > 0
    g = _bench("--full", "--workload", "flux_c2", "--layers", "6", "--steps", "6", "--warmup", "12", "--dense-steps", "0", "--no-cpu-baseline", "--event-period", "1")
    assert all(k["timed_launches"] == k["launches"] for k in g["kernels"].values())


@pytest.mark.parametrize("mode", ["heads", "groups"])
def test_two_rank_line_rehearsed_on_one_gpu(mode):
    """`bench.py --gpus 2` end to end on a one-GPU box (BENCH_SHARE_GPU=1: both ranks on cuda:0, gloo with host staging): the
    launcher, the chunk planner fed by a measured exchange, per-chunk modules with their own slots / query-group offsets, the
    max-over-ranks timing, the exposed-communication probe and rank 0's single line."""
    d = _bench("--full", "--gpus", "2", "--sp-mode", mode, "--grid", "8,12,16", "--layers", "3", "--steps", "3", "--warmup", "3", BENCH_SHARE_GPU="1")
    assert d["n_gpus"] == 2 and d["config"]["dist_world_size"] == 2 and d["config"]["sp_mode"] == mode and d["scaling"] == "strong"
    plan = d["config"]["chunk_plan"]
    assert sum(plan["chunks"]) == (12 if mode == "heads" else 24) and plan["exchange_ms_per_head_measured"] > 0
    assert "rehearsal" in d["config"] and d["cpu_baseline"] is None and d["value"] > 0
    assert 0.0 <= d["exposed_comm"]["exposed_fraction"] <= 1.0


def test_block_loop_with_the_fused_rowwise_pass_equals_the_torch_ops():
    """bench.py's HunyuanBlock chain (double-stream block -> single-stream block -> double-stream block; attention replaced by a fixed
    tensor) with the gated residual + LayerNorm + modulate as chipmunk.residual_ln_modulate -- including the hand-over of the next
    block's LayerNorm + modulate to the previous block's closing residual -- against the same chain on torch's elementwise ops:
    the restructured loop computes the same hidden state (bf16 rounding apart: the fused pass can land one step away, see
    test_residual_ln_modulate_matches_the_reference_sequence)."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    dev = torch.device("cuda:0")
    rows, hid, ffn, heads = 1024, 512, 2048, 4
    torch.manual_seed(3)
    blocks = [bench.HunyuanBlock(kind, dev, hid, ffn, heads) for kind in ("double", "single", "double")]
    x0 = torch.randn(rows, hid, device=dev, dtype=torch.bfloat16)
    attn = [torch.randn(rows, hid, device=dev, dtype=torch.bfloat16) * 0.5 for _ in blocks]

    def run(fused):
        bench.HunyuanBlock.fused_rowwise = fused
        x, xm = x0, None
        with torch.no_grad():
            for i, blk in enumerate(blocks):
                h = blk.pre(x, xm)
                x, xm = blk.post(x, h, attn[i], blocks[i + 1].first_mod() if i + 1 < len(blocks) else None)
        return x

    try:
        a, b = run(True), run(False)
    finally:
        bench.HunyuanBlock.fused_rowwise = True
    torch.cuda.synchronize()
    scale = b.float().abs().max().item()
    assert (a.float() - b.float()).abs().max().item() <= 2.0 ** -5 * scale, ((a.float() - b.float()).abs().max().item(), scale)
    assert ((a.float() - b.float()).abs() <= 2.0 ** -7 * scale).float().mean().item() > 0.99


def test_plain_line_is_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain run (no --full) times the steps and prints the line: no comparators, baseline, legs or per-kernel figures.  Its
    --dump-outputs files are float32, within 64 MB, and bit-identical from run to run: the inputs are seeded, the library's random key
    selection starts from its fixed default seed, and its kernels fold in a fixed order."""
    import numpy as np
    args = ("--grid", "8,12,16", "--layers", "3", "--steps", "3", "--warmup", "3")
    d = _bench(*args, "--dump-outputs", str(tmp_path / "a"))
    _bench(*args, "--dump-outputs", str(tmp_path / "b"))
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"} <= set(d)
    assert d["steps"] == 3 and d["warmup"] == 3 and abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["timed_steps"]["inference_steps"] == [3, 4, 5]        # --steps sets the timed steps; --warmup ran 0, 1, 2 before them
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["dense_gpu_comparator"] is None and d["kernels"] == {}
    assert not any(k.endswith("_leg") for k in d) and "sdpa_flash_libraries" not in d
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) == ["hidden.npy"]
    total = 0
    for name in files:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        total += os.path.getsize(tmp_path / "a" / name)
        assert a.dtype == np.float32 and a.shape == (8 * 12 * 16 + 256, 3072) and np.isfinite(a).all() and np.abs(a).max() > 0
        np.testing.assert_array_equal(a, b)
    assert total <= 64 << 20
