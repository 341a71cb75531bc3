"""The row-relative error metric of the attention tests (helpers.attn_exact / row_rel_err / assert_rows_close), proven on
the CPU: over a fixed list of cases

1. the CPU oracle (the reference's roundings) passes at the shipped bound and its worst row sits at or under
   ORACLE_ROW_ERR (the floor is real and the constant is honest);
2. every mutant -- an exact fp64 output with ONE defect, rounded to bf16 -- fails;
3. ROW_ERR_MARGIN * ORACLE_ROW_ERR is at most half the weakest mutant's error over the whole list (a condition, not a
   measurement: widening the margin later cannot silently re-open the hole).

Mutants come from attn_exact's `keep` / `scale_mul` arguments or from edited index lists; no kernel is involved.
`python tests/test_attn_metric_cpu.py` prints the table of docs/TEST_SENSITIVITY.md (floor per case, error per mutant,
and whether the tolerance the suite used before, assert_close_bf16 against the oracle, accepts the mutant)."""
import functools
import math
import os
import sys

import pytest
import torch

for _p in (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))):
    if _p not in sys.path:
        sys.path.insert(0, _p)             # (run as a script: helpers and the oracle package)

import oracle  # noqa: E402
from helpers import (BF16_EPS, ORACLE_ROW_ERR, ORACLE_ROWSUM_ERR, ROW_ERR_BOUND, ROW_ERR_MARGIN, assert_close_bf16,  # noqa: E402
                     assert_delta_rows_close, assert_rows_close, attn_exact, gathered_matrix_inputs, indicator_v, randn_bf16,
                     random_index_sets, row_rel_err, straddle_inputs)


def _bf16(x):
    return x.to(torch.bfloat16)


def _patterned(pattern, n=1152, H=1):
    """the constructions of test_gpu_attn.py::test_running_max_update_paths"""
    g = torch.Generator().manual_seed(11)
    q, k, v = [torch.randn(1, H, n, 128, generator=g) for _ in range(3)]
    u = torch.randn(128, generator=g)
    u = u / u.norm()
    q = 0.3 * q + 3.0 * u
    if pattern == "ramp":
        k = 0.3 * k + (torch.arange(n).float() / n * 30.0)[None, None, :, None] * u
    else:
        k = 0.3 * k
        k[0, :, 1000] += 40.0 * u
        q[0, :, ::3] *= 0.05
    return _bf16(q), _bf16(k), _bf16(v)


def _dense(nq, nk, seeds, mul=1.0, tol=(2e-2, 2e-2)):
    q, k, v = [randn_bf16(1, 1, n, 128, seed=s) for n, s in zip((nq, nk, nk), seeds)]
    if mul != 1.0:
        q, k = _bf16(q.float() * mul), _bf16(k.float() * mul)
    return dict(q=q, k=k, v=v, tol=tol)


def _gathered(nq, nk, count, seeds, iseed, tol=(2e-2, 2e-2)):
    q, k, v = [randn_bf16(1, 1, n, 128, seed=s) for n, s in zip((nq, nk, nk), seeds)]
    G = math.ceil(nq / 192)
    inds, counts = random_index_sets(1, 1, G, nk, count, nk, seed=iseed)
    return dict(q=q, k=k, v=v, inds=inds, counts=counts, tol=tol)


# name -> inputs; tol = (atol, rtol) of the test that runs this size today
CASES = {
    "dense 1000": lambda: _dense(384, 1000, (1000, 1001, 1002)),
    "dense 4160": lambda: _dense(256, 4160, (64, 4161, 4162)),
    "slice 256 of 32760 keys": lambda: _dense(256, 32760, (1, 2, 3), tol=(1e-2, 2e-2)),
    "slice 256 of 119056 keys": lambda: _dense(256, 119056, (1, 2, 3), tol=(1e-2, 2e-2)),
    "gathered 336 of 1100": lambda: _gathered(576, 1100, 336, (11, 12, 13), 5),
    "gathered 9088 of 20000": lambda: _gathered(384, 20000, 9088, (1, 2, 3), 7),
    "ramp": lambda: dict(zip("qkv", _patterned("ramp")), tol=(2e-2, 2e-2)),
    "spike": lambda: dict(zip("qkv", _patterned("spike")), tol=(2e-2, 2e-2)),
    "q, k x 3": lambda: _dense(384, 1000, (51, 52, 53), mul=3.0),
}
ACCUMULATE_CASE = "gathered 336 of 1100"


def _straddle(align, pattern):
    """the threshold inputs of test_gpu_attn_accuracy.py (dense64's 2 |q| max|k| c against 64), 256 rows of them"""
    q, k, v, _ = straddle_inputs(align, pattern, 64.0, 2.0, 128, 256, 4160, seed=301)
    return dict(q=q[:, :1], k=k[:, :1], v=v[:, :1])


# the other input families the GPU tests run: the oracle's floor on them enters ORACLE_ROW_ERR.  No mutants here: these
# softmaxes are (nearly) one-hot, where most single defects touch keys without mass.
FLOOR_CASES = {
    "dense 1984": lambda: _dense(384, 1984, (384, 1985, 1986)),
    "q, k x 6": lambda: _dense(384, 1000, (51, 52, 53), mul=6.0),
    **{f"threshold, {a} queries, {p}": (lambda a=a, p=p: _straddle(a, p))
       for a in ("random", "along", "against") for p in ("all rows at 0.9", "all rows at 1.1")},
}
# ramp, spike and q, k x 3 concentrate the softmax on a few keys.  A defect that touches only keys of negligible mass (the
# two V rows in the middle of the list, the random key behind the tail) does not change the output there: these INERT pairs
# are printed in the table but are no evidence either way; test_inert_pairs_are_inert checks the stated reason on the exact
# probabilities.  Every other (case, mutant) pair must be rejected.
INERT = {("ramp", "tail read one key too far"), ("ramp", "two V rows swapped"), ("spike", "two V rows swapped"),
         ("q, k x 3", "tail read one key too far")}
# A 1 % scale error on the ramp moves the exact output by 0.008 (the softmax there is a narrow window at the end of the key
# list): it is rejected like every other mutant, but no bound above the oracle's floor could leave it a factor of two
# (0.008 / 2 / 0.0029 = 1.4 < 1.5, the smallest margin), so it alone stays out of the separation minimum.
INPUT_LIMITED = {("ramp", "scale x 1.01")}


def _not_listed(inds, counts, nk):
    """per group one key that its list does not hold (what a tail read one position too far would pick up)"""
    out = []
    for g in range(inds.shape[2]):
        listed = set(inds[0, 0, g, :int(counts[0, 0, g])].tolist())
        out.append(next(j for j in range(nk - 1, -1, -1) if j not in listed))
    return out


@functools.lru_cache(maxsize=None)
def _evaluate(name):
    """exact output, oracle output and the mutants (bf16) of one case"""
    c = CASES[name]()
    q, k, v, inds, counts = c["q"], c["k"], c["v"], c.get("inds"), c.get("counts")
    nq, nk = q.shape[2], k.shape[2]
    exact = attn_exact(q, k, v, inds, counts)
    mut = {}
    if inds is None:
        ref = oracle.dense_attn(q, k, v)[0]
        mid = (nk // 2) // 64 * 64

        def without(a, b):
            keep = torch.ones(nk, dtype=torch.bool)
            keep[a:b] = False
            return attn_exact(q, k, v, keep=keep)
        mut["last key dropped"] = without(nk - 1, nk)
        mut["32-key tile dropped"] = without(mid, mid + 32)
        mut["64-key tile dropped"] = without(mid, mid + 64)
        extra = randn_bf16(1, 1, 2, 128, seed=4242)      # whatever lies behind the last key
        mut["tail read one key too far"] = attn_exact(q, torch.cat([k, extra[:, :, :1]], 2), torch.cat([v, extra[:, :, 1:]], 2))
        a, b = mid + 3, mid + 4
    else:
        ref = oracle.csp_128_attn(q, k, v, inds, counts)
        cnt = int(counts[0, 0, 0])
        mid = (cnt // 2) // 64 * 64

        def without(a, b):
            return attn_exact(q, k, v, torch.cat([inds[..., :a], inds[..., b:]], -1), counts - (b - a))
        mut["last key dropped"] = attn_exact(q, k, v, inds, counts - 1)
        mut["32-key tile dropped"] = without(mid, mid + 32)
        mut["64-key tile dropped"] = without(mid, mid + 64)
        far = inds.clone()
        for g, j in enumerate(_not_listed(inds, counts, nk)):
            far[0, 0, g, cnt] = j
        mut["tail read one key too far"] = attn_exact(q, k, v, far, counts + 1)
        a, b = int(inds[0, 0, 0, mid + 3]), int(inds[0, 0, 0, mid + 4])
    vs = v.clone()
    vs[0, 0, a], vs[0, 0, b] = v[0, 0, b], v[0, 0, a]
    mut["two V rows swapped"] = attn_exact(q, k, vs, inds, counts)
    mut["scale x 1.01"] = attn_exact(q, k, v, inds, counts, scale_mul=1.01)
    mut["scale x 1.05"] = attn_exact(q, k, v, inds, counts, scale_mul=1.05)
    mut["output x 0.9"] = 0.9 * exact
    swapped = exact.clone()
    rows = min(192, nq - 192)
    swapped[:, :, :rows] = exact[:, :, 192:192 + rows]
    mut["group written with its neighbour's result"] = swapped
    return dict(c, exact=exact, ref=ref, touched=(a, b), mut={m: _bf16(x) for m, x in mut.items()})


def _old_tolerance_accepts(o, ref, tol):
    try:
        assert_close_bf16(o, ref, atol=tol[0], rtol=tol[1])
    except AssertionError:
        return False
    return True


@functools.lru_cache(maxsize=None)
def _accumulate():
    """the in-place form on the accumulate case: base -> (oracle result, mutant results), per base magnitude"""
    e = _evaluate(ACCUMULATE_CASE)
    q, k, v, inds, counts, exact = e["q"], e["k"], e["v"], e["inds"], e["counts"], e["exact"]
    rms = float(exact.pow(2).mean().sqrt())
    out = {}
    for base_name, scale in (("unit randn base", 1.0), ("base of the delta's magnitude", rms)):
        base = randn_bf16(*q.shape, seed=99, scale=scale)
        res = base.clone()
        oracle.csp_attn(q, k, v, res, inds, counts, 1)

        def stored(delta):          # bf16 store of the delta, then the bf16 add (the reference's accumulate)
            return _bf16(base.float() + _bf16(delta).float())
        mut = {"delta with the wrong sign": stored(-exact), "delta applied twice": stored(2 * exact)}
        if scale != 1.0:
            mut.update({m: stored(x.double()) for m, x in e["mut"].items()})
        out[base_name] = dict(base=base, res=res, mut=mut)
    return out


def _delta_err(result, base, exact):
    """error of an accumulate result as assert_delta_rows_close judges it (rounding of the stored sum taken off)"""
    err = row_rel_err(result.double() - base.double(), exact)
    return float((err - BF16_EPS * result.double().norm(dim=-1) / exact.norm(dim=-1)).max())


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_passes_and_pins_the_floor(name):
    e = _evaluate(name)
    worst = assert_rows_close(e["ref"], e["exact"], ROW_ERR_BOUND, what=f"oracle, {name}")
    assert worst <= ORACLE_ROW_ERR, f"{name}: the oracle's worst row {worst:.5f} is above ORACLE_ROW_ERR = {ORACLE_ROW_ERR}"


def _floors():
    floors = {n: float(row_rel_err(_evaluate(n)["ref"], _evaluate(n)["exact"]).max()) for n in CASES}
    for n, make in FLOOR_CASES.items():
        c = make()
        floors[n] = float(row_rel_err(oracle.dense_attn(c["q"], c["k"], c["v"])[0], attn_exact(c["q"], c["k"], c["v"])).max())
    e = _evaluate(ACCUMULATE_CASE)
    for base_name, a in _accumulate().items():
        floors[f"in place, {base_name}"] = _delta_err(a["res"], a["base"], e["exact"])
    return floors


@pytest.mark.parametrize("name", list(FLOOR_CASES))
def test_oracle_passes_on_the_other_input_families(name):
    c = FLOOR_CASES[name]()
    worst = assert_rows_close(oracle.dense_attn(c["q"], c["k"], c["v"])[0], attn_exact(c["q"], c["k"], c["v"]), ROW_ERR_BOUND,
                              what=f"oracle, {name}")
    assert worst <= ORACLE_ROW_ERR, f"{name}: the oracle's worst row {worst:.5f} is above ORACLE_ROW_ERR = {ORACLE_ROW_ERR}"


def test_oracle_floor_constant_is_tight():
    """ORACLE_ROW_ERR is the measured maximum (accumulate form included) rounded up to two digits, not a generous guess"""
    floor = max(_floors().values())
    assert floor <= ORACLE_ROW_ERR <= floor + 1e-4, floor


@pytest.mark.parametrize("name", list(CASES))
def test_every_mutant_is_rejected(name):
    e = _evaluate(name)
    for m, o in e["mut"].items():
        if (name, m) in INERT:
            continue
        with pytest.raises(AssertionError, match=r"head 0 group \d+ row \d+"):
            assert_rows_close(o, e["exact"], ROW_ERR_BOUND, what=f"{name}, {m}")


def test_inert_pairs_are_inert():
    """the pairs left out above change nothing for the reason stated: the keys they touch carry under 1e-3 of any row's softmax mass"""
    for name in sorted({n for n, _ in INERT}):
        e = _evaluate(name)
        q, k = e["q"][0, 0].double(), e["k"][0, 0].double()
        p = torch.softmax(q @ k.T / math.sqrt(128), dim=-1)
        a, b = e["touched"]
        if (name, "two V rows swapped") in INERT:
            assert float(p[:, [a, b]].max()) < 1e-3, name
        if (name, "tail read one key too far") in INERT:
            extra = randn_bf16(1, 1, 2, 128, seed=4242)[0, 0, :1].double()
            mass = torch.exp(q @ extra.T / math.sqrt(128))[:, 0] / torch.exp(q @ k.T / math.sqrt(128)).sum(-1)
            assert float(mass.max()) < 1e-3, name


@pytest.mark.parametrize("base_name", ["unit randn base", "base of the delta's magnitude"])
def test_accumulate_form_oracle_passes_and_mutants_fail(base_name):
    e, a = _evaluate(ACCUMULATE_CASE), _accumulate()[base_name]
    worst = assert_delta_rows_close(a["res"], a["base"], e["exact"], 1, ROW_ERR_BOUND, what=f"oracle in place, {base_name}")
    assert worst <= ORACLE_ROW_ERR, worst
    for m, o in a["mut"].items():
        with pytest.raises(AssertionError, match=r"head 0 group \d+ row \d+"):
            assert_delta_rows_close(o, a["base"], e["exact"], 1, ROW_ERR_BOUND, what=f"in place, {base_name}, {m}")


def _mutant_errors():
    errs = {}
    for name in CASES:
        e = _evaluate(name)
        for m, o in e["mut"].items():
            if (name, m) not in INERT | INPUT_LIMITED:
                errs[(name, m)] = float(row_rel_err(o, e["exact"]).max())
    e = _evaluate(ACCUMULATE_CASE)
    for base_name, a in _accumulate().items():
        for m, o in a["mut"].items():
            errs[(f"in place, {base_name}", m)] = _delta_err(o, a["base"], e["exact"])
    return errs


def test_separation_of_bound_and_weakest_mutant():
    assert ROW_ERR_MARGIN in (1.5, 2.0, 3.0)
    errs = _mutant_errors()
    weakest = min(errs, key=errs.get)
    assert ROW_ERR_MARGIN * ORACLE_ROW_ERR <= 0.5 * errs[weakest], (
        f"bound {ROW_ERR_BOUND:.5f} is more than half of the weakest mutant's error {errs[weakest]:.5f} {weakest}")


def test_indicator_v_row_sums_of_the_oracle():
    """with an indicator V every output row of a non-empty group sums to 1; ORACLE_ROWSUM_ERR is how far the oracle's roundings
    (bf16 P against an fp32 normaliser, bf16 output) take it from 1 on the very inputs of test_gpu_attn_accuracy.py's path
    matrix -- the groups that keep 7 and 33 keys set it: few roundings, nothing averages out.  A skipped 32-key tile
    renormalises (the sum stays 1): its column is what gives it away, by a quarter of its value at least."""
    m = gathered_matrix_inputs()
    q, k, inds, counts = m["q"], m["k"], m["inds"], m["counts"]
    nk = k.shape[2]
    live = (counts > 0).repeat_interleave(192, dim=-1)[..., :q.shape[2]]
    worst = {}
    for kind in ("key", "tile", "position"):
        v = m["v_pos"] if kind == "position" else indicator_v(nk, kind).expand(1, 3, nk, 128).contiguous()
        o = oracle.csp_128_attn(q, k, v, m["shared"] if kind == "position" else inds, counts)
        worst[f"gathered, {kind}"] = float((o.double().sum(-1) - 1).abs()[live].max())
    qd, kd = q[:, :1, :384].contiguous(), k[:, :1, :4160].contiguous()
    v = indicator_v(4160, "tile")[None, None]
    worst["dense, tile"] = float((oracle.dense_attn(qd, kd, v)[0].double().sum(-1) - 1).abs().max())
    keep = torch.ones(4160, dtype=torch.bool)
    keep[2048:2080] = False
    full, cut = attn_exact(qd, kd, v), attn_exact(qd, kd, v, keep=keep)
    col = (2048 // 32) % 128
    assert float((_bf16(cut).double()[..., col] - full[..., col]).abs().min()) > 0.25 * float(full[..., col].min())
    print("oracle row-sum deviation:", worst)
    top = max(worst.values())
    assert top <= ORACLE_ROWSUM_ERR <= top + 1e-4, worst


if __name__ == "__main__":
    print("| case | oracle floor | mutant | row error | old tolerance |")
    print("|---|---|---|---|---|")
    for name in CASES:
        e = _evaluate(name)
        floor = float(row_rel_err(e["ref"], e["exact"]).max())
        for m, o in e["mut"].items():
            acc = "accepts" if _old_tolerance_accepts(o, e["ref"], e["tol"]) else "rejects"
            note = " (inert on this input)" if (name, m) in INERT else " (input-limited)" if (name, m) in INPUT_LIMITED else ""
            print(f"| {name} | {floor:.4f} | {m}{note} | {float(row_rel_err(o, e['exact']).max()):.4f} | {acc} (atol {e['tol'][0]:g}) |")
    e = _evaluate(ACCUMULATE_CASE)
    for base_name, a in _accumulate().items():
        floor = _delta_err(a["res"], a["base"], e["exact"])
        for m, o in a["mut"].items():
            acc = "accepts" if _old_tolerance_accepts(o, a["res"], (3e-2, 2e-2)) else "rejects"
            print(f"| in place, {base_name} | {floor:.4f} | {m} | {_delta_err(o, a['base'], e['exact']):.4f} | {acc} (atol 0.03) |")
    print("\nfloor on the other input families:", {n: round(f, 4) for n, f in _floors().items() if n in FLOOR_CASES})
    errs = _mutant_errors()
    weakest = min(errs, key=errs.get)
    print(f"\nweakest mutant {weakest}: {errs[weakest]:.4f}; bound {ROW_ERR_BOUND:.4f}")
