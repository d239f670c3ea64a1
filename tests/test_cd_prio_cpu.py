"""CPU-only checks around RCPPML_OPT_CD_PRIO: the option constant, the default and the accepted range agree between
include/rcppml_gpu.h, the library's own check (common.hip.h) and rcppml_amd/_abi.py; an out-of-range value is refused before it
reaches the library; and the inputs of tests/test_gpu_cd_prio.py spread the sweep counts as that test needs (float64 restatement
of the solve, tests/cd_ref.py)."""
import os
import re

import numpy as np
import pytest

from tests import cd_prio_inputs as pi
from tests.cd_ref import cd_solve_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()


def test_option_constant_and_default_agree_with_the_header():
    from rcppml_amd import _abi
    src = _header()
    opts = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(RCPPML_OPT_\w+)\s*=\s*(\d+)", src)}
    assert opts["RCPPML_OPT_CD_PRIO"] == _abi.OPT_CD_PRIO
    assert opts["RCPPML_OPT_CD_PLACED"] == _abi.OPT_CD_PLACED and opts["RCPPML_OPT_CD_ASSUME_CUS"] == _abi.OPT_CD_ASSUME_CUS
    assert len(set(opts.values())) == len(opts)                         # no two options share a number
    default = int(re.search(r"#define\s+RCPPML_CD_PRIO_DEFAULT\s+(\d+)", src).group(1))
    assert default == _abi.CD_PRIO_DEFAULT and _abi.cd_prio_valid(default)


def test_accepted_range_agrees_with_the_library_check():
    from rcppml_amd import _abi
    src = open(os.path.join(ROOT, "rcppml_amd", "csrc", "common.hip.h")).read()
    body = re.search(r"inline bool rcppml_cd_prio_valid\(int v\)\s*\{\s*return (.*?);\s*\}", src).group(1)
    expr = body.replace("&&", " and ")
    for v in range(-3, 80):
        assert bool(eval(expr, {"v": v})) == _abi.cd_prio_valid(v), v
    ok = [v for v in range(-3, 80) if _abi.cd_prio_valid(v)]
    assert ok == sorted(h + 8 * w for h in _abi.CD_PRIO_MODES for w in _abi.CD_PRIO_MODES)
    assert _abi.cd_prio_value(3, 2) == 19


def test_out_of_range_value_is_refused():
    from rcppml_amd import _abi
    for h, w in ((5, 0), (0, 5), (-1, 0), (8, 0)):
        with pytest.raises(ValueError):
            _abi.cd_prio_value(h, w)

    class NoHandle:                                 # refused before the handle is read: no context (and no GPU) needed
        @property
        def _h(self):
            raise AssertionError("the library must not be reached")

    for bad in (-1, 5, 6, 7, 40, 37, 64, 1 << 20, 1.0, None):
        with pytest.raises(_abi.BackendError):
            _abi.Context.set_option(NoHandle(), _abi.OPT_CD_PRIO, bad)


@pytest.mark.parametrize("n,k", [(n, k) for _, n in pi.PLACED_SHAPES for k in pi.KS] + [(n, k) for n in pi.TILE_PER_WAVE_NS for k in pi.KS])
def test_inputs_spread_the_sweep_counts(n, k):
    G, B, X0 = pi.problem(n, k)
    _, sw, _ = cd_solve_batch(G, B, X0, warm=True, maxit=pi.MAXIT, tol=float(np.float32(pi.TOL)))
    assert sw.min() >= 1 and sw.min() <= 5 and sw.max() == pi.MAXIT
    assert np.sum((sw > 5) & (sw < pi.MAXIT)) >= n // 10            # and a middle: columns freeze at different sweeps
