// cd_placement.hip.h -- the static tile -> (SIMD, wave) map of the explicitly placed CD-solve launch (cd_mfma_placed_kernel).
//
// A SIMD's waves share its VALU + f32-MFMA issue, so a SIMD is busy for the SUM of its tiles' sweeps and the kernel lasts as
// long as the fullest SIMD.  With one workgroup of 4 R waves per CU, wave w of workgroup b serves SIMD class s = w & 3 of that CU
// in round r = w >> 2 (the waves of a class share a SIMD; global index g = 4 b + s), and the tiles -- numbered in longest-first work order -- are dealt out in closed
// form: round r takes positions [r S, (r + 1) S), ascending in g for the rounds whose bit in `desc` is clear and descending for
// the others; the T - R S tiles left over (the shortest) go one each to the last-round wave of the SIMDs from the far end
// (`extra_top`) or the near end of g, which runs them after its own.  No atomics, no queue: the map is a function of (g, r).
// tools/cd_placement_model.py restates these functions and evaluates the per-SIMD sums on recorded sweep counts.
#pragma once
#include <cstdint>

namespace rk {

struct CdPlace {
    int simds;       // S = 4 x workgroups
    int rounds;      // R = resident waves per SIMD
    int desc;        // bit r set: round r is dealt in descending SIMD order
    int extra_top;   // 1: left-over tile e goes to SIMD S - 1 - e, 0: to SIMD e
};

// the map found best by tools/cd_placement_model.py on the recorded C2 sweep counts (tests/golden/cd_tile_sweeps_c2.json)
constexpr int CD_PLACE_DESC = 0x6;          // rounds: up, down, down, up
constexpr int CD_PLACE_EXTRA_TOP = 0;       // left-over tiles beside the longest round-0 tiles (whose rounds 1 and 2 are the shortest)

// work-order position of the tile that SIMD g runs in round r
__host__ __device__ inline int64_t cd_place_pos(const CdPlace& pl, int g, int r) {
    return (int64_t)r * pl.simds + (((pl.desc >> r) & 1) ? pl.simds - 1 - g : g);
}
// first left-over index of SIMD g (its last-round wave takes e, e + S, ... while R S + e < T)
__host__ __device__ inline int64_t cd_place_extra(const CdPlace& pl, int g) { return pl.extra_top ? pl.simds - 1 - g : g; }

// rcppml_hip_order_columns lays every second group of 16 x 128 slots out in reverse (the serpentine of order_scatter_body,
// kernels.hip.h): tile position p of the longest-first order -> the tile that holds it.  `tpb` = tiles per 128 slots.  An
// involution on the tiles of whole groups, the identity elsewhere.
__host__ __device__ inline int64_t cd_place_unserp(int64_t p, int tpb, int64_t ncols) {
    const int64_t blk = p / tpb, grp = blk >> 4;
    if ((grp & 1) && (grp + 1) * 16 <= (ncols >> 7)) return (((grp << 4) + 15 - (blk & 15)) * tpb) + p % tpb;
    return p;
}

}  // namespace rk
