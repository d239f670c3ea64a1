#!/usr/bin/env python
"""CPU model of where the tiles of a CD solve run, and what the fullest SIMD carries.

The MFMA CD kernels solve one tile of columns (32 or 16) per wave, and a wave runs until its slowest column has converged: a
tile costs its MAXIMUM sweep count.  The waves of a SIMD share its VALU + f32-MFMA issue, so a SIMD is busy for the sum of its
tiles' costs and the kernel lasts as long as the fullest SIMD.  This tool takes the per-tile maxima of one solve, numbered in
longest-first work order, and evaluates that sum per SIMD for

  (a) the tile-per-wave launch: workgroups of four tiles in the serpentine layout of rcppml_hip_order_columns (every second
      whole group of 16 x 128 slots reversed), dealt round-robin to the CUs, `resident` workgroups per CU at once; the surplus
      workgroups go, in order, to the CU that has the least work so far (greedy: the first to free a slot); wave w of a
      workgroup sits on SIMD w & 3;
  (b) the explicitly placed launch: the closed-form map of rcppml_amd/csrc/cd_placement.hip.h, restated in place_pos() /
      place_extra() below: round r of SIMD g takes position r S + g (ascending rounds) or r S + S - 1 - g (descending ones),
      left-over tile e goes to SIMD S - 1 - e (or e).

    python tools/cd_placement_model.py [tests/golden/cd_tile_sweeps_c2.json] [--cus 256]

prints max / mean load and the load of the SIMD that holds the longest tile for both, for every choice of the free rounds'
direction, and the predicted gain of the best map over (a).
"""
import argparse
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cd_tile_sweeps_c2.json")
# the map the library ships (CD_PLACE_DESC / CD_PLACE_EXTRA_TOP in cd_placement.hip.h)
SHIPPED_DESC, SHIPPED_EXTRA_TOP = 0x6, 0


def serpentine_tile(p, tiles_per_128, ncols):
    """Tile that holds longest-first tile position p in the layout of rcppml_hip_order_columns (cd_place_unserp)."""
    blk, grp = p // tiles_per_128, (p // tiles_per_128) >> 4
    if (grp & 1) and (grp + 1) * 16 <= (ncols >> 7):
        return ((grp << 4) + 15 - (blk & 15)) * tiles_per_128 + p % tiles_per_128
    return p


def place_pos(simds, desc, g, r):
    return r * simds + (simds - 1 - g if (desc >> r) & 1 else g)


def place_extra(simds, extra_top, g):
    return simds - 1 - g if extra_top else g


def placed_map(ntiles, cus, rounds, desc=SHIPPED_DESC, extra_top=SHIPPED_EXTRA_TOP):
    """[(simd, [positions it runs])] of the explicitly placed launch: what cd_mfma_placed_kernel's waves loop over."""
    simds = 4 * cus
    out = [[] for _ in range(simds)]
    for g in range(simds):
        for r in range(rounds):
            p = place_pos(simds, desc, g, r)
            if p < ntiles:
                out[g].append(p)
        e = place_extra(simds, extra_top, g)
        while rounds * simds + e < ntiles:
            out[g].append(rounds * simds + e)
            e += simds
    return out


def rounds_for(ntiles, cus, tile_cols=32):
    """Waves per SIMD of the placed launch: tiles per SIMD rounded down (32-column tiles: 1..4, the rest are left-over tiles);
    16-column tiles: two rounds once there are more tiles than SIMDs (the surplus tiles are the second round)."""
    if tile_cols == 16:
        return 2 if ntiles > 4 * cus else 1
    return max(1, min(4, ntiles // (4 * cus)))


def load_placed(tile_max, cus, rounds=None, desc=SHIPPED_DESC, extra_top=SHIPPED_EXTRA_TOP):
    tile_max = np.asarray(tile_max, np.int64)
    rounds = rounds or rounds_for(len(tile_max), cus)
    return np.array([tile_max[ps].sum() if ps else 0 for ps in placed_map(len(tile_max), cus, rounds, desc, extra_top)], np.int64)


def load_present(tile_max, cus, tile_cols, ncols, resident, serpentine=True):
    """Per-SIMD load of the tile-per-wave launch (workgroups of four tiles) under round-robin dispatch with `resident`
    workgroups per CU (0: every workgroup is resident at once, plain round-robin)."""
    tile_max = np.asarray(tile_max, np.int64)
    nt = len(tile_max)
    layout = np.zeros(nt, np.int64)                 # cost of the tile stored at each layout slot
    for p in range(nt):
        layout[serpentine_tile(p, 128 // tile_cols, ncols) if serpentine else p] = tile_max[p]
    nwg = (nt + 3) // 4
    load = np.zeros((cus, 4), np.int64)
    first = nwg if resident <= 0 else min(nwg, cus * resident)
    for i in range(nwg):
        cu = i % cus if i < first else int(np.argmin(load.sum(axis=1)))
        t = layout[4 * i:4 * i + 4]
        load[cu, :len(t)] += t
    return load.reshape(-1)


def report(name, load, where_longest):
    mean = load.mean()
    print("  %-34s max %5d  mean %8.2f  max/mean %.4f  SIMD of the longest tile %5d" % (name, load.max(), mean, load.max() / mean, load[where_longest]))
    return load.max() / mean


def longest_simd_present(tile_max, cus, tile_cols, ncols, resident):
    p = int(np.argmax(tile_max))
    t = serpentine_tile(p, 128 // tile_cols, ncols)
    wg = t // 4
    # (the longest tile is in the first dispatch round for every shape looked at here)
    return (wg % cus) * 4 + (t & 3)


def model_side(name, side, cus):
    tm = np.asarray(side["tile_max"], np.int64)
    tile_cols, ncols = side["tile_cols"], side["ncols"]
    simds = 4 * cus
    per = len(tm) / simds
    resident = int(per) if (1.0 < per < 4.0 and per - int(per) < 0.5 and tile_cols == 32) else 0   # cd_mfma_launch's cap; the 16-column launch has none
    print("%s side: %d tiles of %d columns on %d SIMDs (%.2f per SIMD), lower bound max/mean 1.0 = %.1f sweeps" % (name, len(tm), tile_cols, simds, per, tm.sum() / simds))
    a = load_present(tm, cus, tile_cols, ncols, resident)
    ra = report("present (resident %d)" % resident, a, longest_simd_present(tm, cus, tile_cols, ncols, resident))
    if resident:
        report("present, no residency cap", load_present(tm, cus, tile_cols, ncols, 0), longest_simd_present(tm, cus, tile_cols, ncols, 0))
    rounds = rounds_for(len(tm), cus, tile_cols)
    best = None
    for desc_hi in range(1 << max(0, rounds - 2)):
        desc = 0x2 | (desc_hi << 2)
        for extra_top in (1, 0):
            b = load_placed(tm, cus, rounds, desc, extra_top)
            pm = placed_map(len(tm), cus, rounds, desc, extra_top)
            g0 = next(g for g, ps in enumerate(pm) if int(np.argmax(tm)) in ps)
            rb = report("placed desc=0x%x extra_top=%d" % (desc, extra_top), b, g0)
            if best is None or b.max() < best[0]:
                best = (b.max(), desc, extra_top, rb)
    print("  best placed map: desc=0x%x extra_top=%d; predicted gain over the present layout %.2f %% (max load %d -> %d)" % (
        best[1], best[2], 100.0 * (1.0 - best[0] / a.max()), a.max(), best[0]))
    return a.max(), best


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file", nargs="?", default=GOLDEN, help="JSON: {side: {tile_cols, ncols, tile_max: [per-tile maximum sweep counts, longest-first work order]}}")
    ap.add_argument("--cus", type=int, default=256)
    args = ap.parse_args()
    with open(args.file) as f:
        sides = json.load(f)
    for name in sorted(sides):
        if isinstance(sides[name], dict) and "tile_max" in sides[name]:
            model_side(name, sides[name], args.cus)


if __name__ == "__main__":
    main()
