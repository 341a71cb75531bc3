"""The tile maps of the sparse-MLP GEMMs (chipmunk_amd/csrc/mlp.hip: plan_tiles / tile_at / mm1_kernel's walk, mm2_kernel's map) written out
in Python, for a launch over B sequences: the map runs over B * G groups, G = ceil(M / 128); group g is group g % G of sequence g // G.

It is the kernels' integer arithmetic, statement by statement, so that the properties a launch relies on -- every live unit of work is
produced exactly once, nothing else is -- can be checked over many shapes without a GPU (tests/test_mlp_batched_host.py, which also ties the
constants below to the source)."""

BM = 128         # rows per group
XCDS = 8         # block b runs on XCD b % 8
GEMM1_BN = 128   # the shipped GEMM1 form <128, 64, 2, 2>: 128 packed columns per tile, two workgroups per CU
GEMM1_WPS = 2
GEMM2_BN = 256   # the shipped GEMM2 form <256, 32, 3, 2, 8>
NR = 4           # column tiles per block of the "NR column tiles x all groups" walk (options mm1_nr / mm2_nr unset)


def nsub(bn):
    """64 x 64 sub-tiles per GEMM1 tile (NSUB in mm1_kernel, 4-wave form)"""
    return 2 * (bn // 64)


def sequence_of(g, G):
    """group of the launch -> (sequence, group inside it)"""
    b = g // G
    return b, g - b * G


def plan_tiles(counts, n_groups, nt_max, nr, xcd, bn, slots_per_xcd=0, n_sub=1):
    cmax = max(counts[:n_groups]) if n_groups else 0
    pl = dict(G=n_groups, NR=nr, nsub=n_sub)
    pl["NTl"] = min((cmax + bn - 1) // bn, nt_max)
    total = pl["NTl"] * n_groups
    q, r = total >> 3, total & 7
    pl["mine"] = q + (1 if xcd < r else 0)
    pl["full"] = pl["mine"]
    if n_sub > 1 and slots_per_xcd > 0:
        rem = pl["mine"] % slots_per_xcd
        if pl["mine"] > slots_per_xcd and rem > 0 and rem * n_sub <= slots_per_xcd:
            pl["full"] = pl["mine"] - rem
    pl["base"] = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    pl["slots"] = pl["full"] + (pl["mine"] - pl["full"]) * n_sub
    return pl


def tile_at(pl, slot):
    """-> (g, nt, sub, live); sub < 0: whole tile"""
    sub = -1
    if slot >= pl["full"]:
        k = slot - pl["full"]
        sub = k % pl["nsub"]
        slot = pl["full"] + k // pl["nsub"]
    live = slot < pl["mine"]
    t = pl["base"] + slot
    per = pl["G"] * pl["NR"]
    nb = t // per
    rem = t - nb * per
    nr = min(pl["NR"], pl["NTl"] - nb * pl["NR"])
    g = rem // nr if nr > 0 else 0
    nt = nb * pl["NR"] + (rem - g * nr if nr > 0 else 0)
    return g, nt, sub, live


def gemm1_launch(counts, B, M, F, cus, split=True):
    """What one GEMM1 launch computes: a list of (sequence, group, column tile, sub-tile) with sub-tile in 0..3 -- a whole tile is listed as
    the sub-tiles it covers.  `counts`: B * G numbers.  Mirrors launch_mm1_variant (grid, slots) and mm1_kernel (the walk and its skips).
    Also returns the number of units that came from the tail split."""
    bn, G = GEMM1_BN, (M + BM - 1) // BM
    n_groups = B * G
    nt_max = (F + bn - 1) // bn
    nr = min(NR, nt_max)
    resident = GEMM1_WPS * cus // XCDS
    slots_per_xcd = resident if split else 0
    tiles_per_xcd = (n_groups * nt_max + 7) // 8
    per_xcd = min(tiles_per_xcd, resident)
    grid = per_xcd * XCDS
    out, from_split = [], 0

    def units(b, g, nt, subs):
        for sub in subs:
            n0 = nt * bn + (sub >> 1) * 64
            if n0 >= counts[b * G + g] or g * BM + (sub & 1) * 64 >= M:
                continue
            yield (b, g, nt, sub)

    for block in range(grid):
        pl = plan_tiles(counts, n_groups, nt_max, nr, block & 7, bn, slots_per_xcd, nsub(bn))
        stride = grid >> 3
        slot = block >> 3
        while slot < pl["slots"]:
            g_all, nt, sub, live = tile_at(pl, slot)
            slot += stride
            if not live:
                continue
            b, g = sequence_of(g_all, G)
            cnt = counts[g_all]
            if sub < 0:
                if nt * bn >= cnt:
                    continue
                out.extend(units(b, g, nt, range(4)))
            else:
                new = list(units(b, g, nt, [sub]))
                from_split += len(new)
                out.extend(new)
    return out, from_split


def gemm1_live(counts, B, M):
    """The units of work a GEMM1 launch has to produce."""
    bn, G = GEMM1_BN, (M + BM - 1) // BM
    out = []
    for b in range(B):
        for g in range(G):
            cnt = counts[b * G + g]
            for nt in range((cnt + bn - 1) // bn):
                for sub in range(4):
                    if nt * bn + (sub >> 1) * 64 < cnt and g * BM + (sub & 1) * 64 < M:
                        out.append((b, g, nt, sub))
    return out


def gemm2_launch(counts, B, M, N2, cus, order=True):
    """What one GEMM2 launch computes: (sequence, group, column tile of N2) per workgroup that does not exit early.  Mirrors
    launch_mm2_variant and mm2_kernel's map, the length-aware placement of a one-round launch included."""
    bn, Gs = GEMM2_BN, (M + BM - 1) // BM
    G = B * Gs
    NT = (N2 + bn - 1) // bn
    nr_ = min(NR, NT)
    cap = cus // XCDS if order else 0
    grid = ((G * NT + 7) // 8) * 8
    xcdq, xcdr = (G * NT) >> 3, (G * NT) & 7
    out = []

    def group_of(tt):
        nb_ = tt // (G * nr_)
        rem_ = tt - nb_ * (G * nr_)
        return rem_ // min(nr_, NT - nb_ * nr_)

    for block in range(grid):
        xcd, slot = block & 7, block >> 3
        mine = xcdq + (1 if xcd < xcdr else 0)
        if slot >= mine:
            continue
        tbase = xcd * (xcdq + 1) if xcd < xcdr else xcdr * (xcdq + 1) + (xcd - xcdr) * xcdq
        t = tbase + slot
        if cap > 0 and cap < mine <= 64 and mine <= 2 * cap:
            nl = 2 * cap - mine
            want = nl + slot if slot < mine - cap else slot - (mine - cap) if slot < cap else mine - 1 - (slot - cap)
            lens = [counts[group_of(tbase + lane)] for lane in range(mine)]
            hit = None
            for lane in range(mine):
                rank = sum(1 for j in range(mine) if lens[j] > lens[lane] or (lens[j] == lens[lane] and j < lane))
                if rank == want:
                    assert hit is None
                    hit = lane
            t = tbase + hit
        nb = t // (G * nr_)
        rem = t - nb * (G * nr_)
        nr = min(nr_, NT - nb * nr_)
        gi = rem // nr
        nt = nb * nr_ + rem - gi * nr
        if counts[gi] == 0:
            continue
        b, g = sequence_of(gi, Gs)
        out.append((b, g, nt))
    return out


def gemm2_live(counts, B, M, N2):
    Gs = (M + BM - 1) // BM
    NT = (N2 + GEMM2_BN - 1) // GEMM2_BN
    return [(b, g, nt) for b in range(B) for g in range(Gs) for nt in range(NT) if counts[b * Gs + g] > 0]
