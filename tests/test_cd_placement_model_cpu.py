"""tools/cd_placement_model.py on the recorded per-tile sweep maxima of one steady-state c2 iteration
(tests/golden/cd_tile_sweeps_c2.json): the static map of the explicitly placed CD launch covers every tile exactly once, and
its modelled load of the fullest SIMD is not above that of the launch it replaces."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("cd_placement_model", os.path.join(ROOT, "tools", "cd_placement_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _model()
with open(M.GOLDEN) as _f:
    SIDES = json.load(_f)


def test_model_restates_the_shipped_map():
    src = open(os.path.join(ROOT, "rcppml_amd", "csrc", "cd_placement.hip.h")).read()
    assert int(re.search(r"CD_PLACE_DESC = (0x[0-9a-fA-F]+)", src).group(1), 16) == M.SHIPPED_DESC
    assert int(re.search(r"CD_PLACE_EXTRA_TOP = (\d)", src).group(1)) == M.SHIPPED_EXTRA_TOP


@pytest.mark.parametrize("side,ntiles", [("H", 3125), ("W", 1250)])
def test_fixture_shape(side, ntiles):
    s = SIDES[side]
    assert len(s["tile_max"]) == ntiles == (s["ncols"] + s["tile_cols"] - 1) // s["tile_cols"]
    assert min(s["tile_max"]) >= 1 and max(s["tile_max"]) <= 100


@pytest.mark.parametrize("ntiles,cus,tile_cols", [(3125, 256, 32), (1250, 256, 16), (26, 2, 32), (130, 2, 32), (1, 2, 32), (8, 2, 32),
                                                 (51, 2, 16), (9, 2, 16), (4, 2, 16), (4096, 256, 32), (5119, 256, 32)])
def test_every_tile_exactly_once(ntiles, cus, tile_cols):
    rounds = M.rounds_for(ntiles, cus, tile_cols)
    for desc in (0x2, 0x6, 0xA, 0xE):
        for extra_top in (0, 1):
            pm = M.placed_map(ntiles, cus, rounds, desc, extra_top)
            assert len(pm) == 4 * cus
            assert sorted(p for ps in pm for p in ps) == list(range(ntiles))


@pytest.mark.parametrize("tiles_per_128,ncols", [(4, 100000), (8, 20000), (4, 805), (4, 4133), (8, 4133)])
def test_serpentine_is_an_involution_on_the_tiles(tiles_per_128, ncols):
    cols = 128 // tiles_per_128
    nt = (ncols + cols - 1) // cols
    t = [M.serpentine_tile(p, tiles_per_128, ncols) for p in range(nt)]
    assert sorted(t) == list(range(nt))
    assert [M.serpentine_tile(q, tiles_per_128, ncols) for q in t] == list(range(nt))


@pytest.mark.parametrize("side", ["H", "W"])
def test_placed_map_is_not_worse_than_the_present_layout(side):
    s = SIDES[side]
    tm, cus = np.asarray(s["tile_max"]), 256
    per = len(tm) / (4 * cus)
    resident = int(per) if (s["tile_cols"] == 32 and 1.0 < per < 4.0 and per - int(per) < 0.5) else 0
    present = M.load_present(tm, cus, s["tile_cols"], s["ncols"], resident)
    placed = M.load_placed(tm, cus, M.rounds_for(len(tm), cus, s["tile_cols"]))
    assert present.sum() == placed.sum() == tm.sum()
    assert placed.max() / placed.mean() <= present.max() / present.mean()
