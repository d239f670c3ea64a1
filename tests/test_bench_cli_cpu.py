"""bench.py's command line without a GPU: a plain run is the default, --full opts into the figures beyond the headline, and the
options that skip single --full legs still parse beside it."""
import sys

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert a.full is False and (a.steps, a.warmup, a.gpus) == (20, 5, 1)
    assert (a.rows, a.cols, a.density, a.k) == (20000, 100000, 0.01, 64)


def test_full_and_its_skips(monkeypatch):
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--no-plugin-figure", "--no-cpu-ref", "--no-fp64-leg", "--no-noop-count")
    assert a.full and a.no_cpu_baseline and a.no_plugin_figure and a.no_cpu_ref and a.no_fp64_leg and a.no_noop_count
