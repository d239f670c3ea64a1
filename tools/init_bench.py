#!/usr/bin/env python3
"""tools/init_bench.py -- does the SVD-seeded start of nmf(seed = "lanczos") pay for itself?  (rcppml_gpu_nmf_svd_init_ex,
csrc/ops_svd.hip; the start kernel: nmf_start_kernel, csrc/kernels_svd.hip.h.)

Fits: the hawaiibirds and movielens fixtures and tests/golden/pbmc3k.spz, k in {10, 32}, tol = 1e-4, maxit = 100, fp32 and fp64, each
from seed = <int> (--seed, default 42: the random start) and from seed = "lanczos" with svd_seed = the same integer.  Per fit, after
one warm-up call: iterations to convergence, the final loss, and the wall time of the whole nmf() call (median of --repeat, default
3).  The "lanczos" leg's wall time counts the start (the Lanczos run, the start kernel, the one download of k (m + n) values); the
start's own init_wall_ms and Lanczos steps are reported beside it.  `pays` says whether the SVD-seeded call was the faster one.

Kernel: on pbmc3k's two sides at k = 32 (the step count of that start), device milliseconds of the one nmf_start_kernel launch
beside the ritz_kernel launch it replaces (rcppml_hip_nmf_start_time: medians of 20 launches after a warm-up, between two events
on the stream), and the host milliseconds of what the Ritz path needs on top: |.| sqrt(sigma) and the transpose to k x len in numpy.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from rcppml_amd import _abi, nmf as N  # noqa: E402
from rcppml_amd.data import CSC  # noqa: E402


def fixture(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return CSC(tuple(int(v) for v in z["shape"]), z["p"].astype(np.int32), z["i"].astype(np.int32), z["x"].astype(np.float64))


def pbmc3k():
    from oracle import oracle as O
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    _, m, n, _, _ = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    return CSC((m, n), np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64))


def fit_leg(A, k, precision, seed, repeat, **kw):
    call = lambda: N.nmf(A, k, tol=1e-4, maxit=100, seed=seed, precision=precision, **kw)      # noqa: E731
    call()                                               # warm-up
    ts, mod = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        mod = call()
        ts.append((time.perf_counter() - t0) * 1e3)
    out = dict(iter=int(mod.misc["iter"]), loss=float(mod.misc["loss"]), wall_ms=statistics.median(ts))
    if "init" in mod.misc:
        out.update(init_wall_ms=float(mod.misc["init_wall_ms"]), init_steps=int(mod.misc["init_iters"]), init_k_svd=int(mod.misc["init_k_svd"]))
    return out


def kernel_leg(A, k, steps, repeat=20):
    out = {}
    rng = np.random.default_rng(0)
    for precision, dt in (("float", np.float32), ("double", np.float64)):
        for side, length in (("W", A.rows), ("H", A.cols)):
            start_ms, ritz_ms = _abi.nmf_start_time(length, steps, k, k, precision=precision, reps=repeat)
            # what the Ritz path adds on the host: the download comes back as doubles, len x k column by column
            U = rng.standard_normal((k, length)).T
            d = np.abs(rng.standard_normal(k)) + 1.0
            ts = []
            for _ in range(repeat + 1):
                t0 = time.perf_counter()
                np.ascontiguousarray(np.abs(U.astype(dt)) * np.sqrt(d.astype(dt)), dtype=np.float64)
                ts.append((time.perf_counter() - t0) * 1e3)
            out["%s_%s" % (side, precision)] = dict(len=length, steps=steps, start_kernel_ms=start_ms, ritz_kernel_ms=ritz_ms,
                                                    ritz_host_transform_ms=statistics.median(ts[1:]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--only", default="", help="comma-separated subset of hawaiibirds, movielens, pbmc3k")
    a = ap.parse_args()
    sets = dict(hawaiibirds=lambda: fixture("hawaiibirds"), movielens=lambda: fixture("movielens"), pbmc3k=pbmc3k)
    names = [s for s in a.only.split(",") if s] or list(sets)
    fits, steps32 = [], None
    for name in names:
        A = sets[name]()
        for k in (10, 32):
            for precision in ("fp32", "fp64"):
                rnd = fit_leg(A, k, precision, a.seed, a.repeat)
                svd = fit_leg(A, k, precision, "lanczos", a.repeat, svd_seed=a.seed)
                fits.append(dict(data=name, m=A.rows, n=A.cols, nnz=int(A.x.shape[0]), k=k, precision=precision, random=rnd, lanczos=svd,
                                 pays=bool(svd["wall_ms"] < rnd["wall_ms"])))
                if name == "pbmc3k" and k == 32:
                    steps32 = svd["init_steps"]
        if name == "pbmc3k":
            kern = kernel_leg(A, 32, steps32)
    res = dict(tool="init_bench", tol=1e-4, maxit=100, seed=a.seed, repeat=a.repeat, fits=fits)
    if "pbmc3k" in names:
        res["kernel_pbmc3k_k32"] = kern
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
