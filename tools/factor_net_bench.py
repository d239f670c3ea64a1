#!/usr/bin/env python3
"""tools/factor_net_bench.py -- a multi-layer factor graph resident on the device (csrc/ops_graph.hip) against the same fit done one
plugin call per layer and outer iteration, the only way the plugin could run it before (and what the reference's GPU path does
through this plugin: graph/fit.hpp:264-375 calls nmf() per layer with max_iter = 1).
Workload: pbmc3k (tests/golden/pbmc3k.spz), a 3-layer chain k = 32 -> 16 -> 8, max_iter = 20, tol = 0, Cholesky, fp64, warm-up
included on both sides.
  resident   one call of rcppml_gpu_factor_net_fit_ex
  per_call   the warm-up and every outer iteration as separate entry calls -- rcppml_gpu_nmf_ex for the sparse first layer,
             rcppml_gpu_nmf_dense_unified_double for the dense ones -- with the states carried through the host, the effective
             inputs transposed there, and the layers' losses summed in numpy as the reference does on the CPU
Each side: one warm-up run, then the median of --reps timed runs (wall clock of the whole call, uploads and downloads included);
the per-call side also reports how its last run splits into the host's loss pass and everything else (the entry calls).
Also: the entry's device-op calls and own kernel launches per outer iteration, the relative difference of the two sides' final
loss, and the numpy float64 restatement (tests/factor_net_ref.py) timed once on a --numpy-iters fit (it is a specification, not a
tuned CPU code).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from rcppml_amd import _abi, data  # noqa: E402

RANKS = (32, 16, 8)


def pbmc3k():
    from oracle import oracle as O
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    _, m, n, _, _ = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    return data.CSC((m, n), np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64))


def median_of(fn, reps):
    r = fn()                                             # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, statistics.median(ts), ts


def graph_args():
    L = len(RANKS)
    return dict(rank=list(RANKS), src_kind=[0] + [1] * (L - 1), branches=[[]] + [[i] for i in range(L - 1)], cond_Z=[None] * L,
                L1=[(0.0, 0.0)] * L, L2=[(0.0, 0.0)] * L, upper_bound=[(0.0, 0.0)] * L, nonneg=[(True, True)] * L)


def resident(A, max_iter, seed):
    m, n = A.shape
    return _abi._check(_abi.factor_net_fit(A, None, m, n, **graph_args(), max_iter=max_iter, tol=0.0, seed=seed, solver_mode=1), "factor graph fit")


def layer_call(A, X, k, W_T, H, iters):
    """One existing plugin call on layer data (the CSC for the first layer, a dense array otherwise): W_T, H updated in place."""
    if X is None:
        m, n = A.shape
        r = _abi.nmf_unified(A.p, A.i, A.x, m, n, k, W_T, H, entry="ex", max_iter=iters, tol=0.0, solver_mode=1, sort_model=0,
                             precision=_abi.F64)
    else:
        r = _abi.nmf_dense(X, k, W_T, H, entry="double", max_iter=iters, tol=0.0, solver_mode=1)
    _abi._check(r, "per-call layer fit")
    return r["d"]


def per_call(A, dense, max_iter, seed, split=None):
    """fit_deep with one plugin call per layer fit; returns the summed loss of the last outer iteration.  split (a dict): the
    seconds spent inside the entry calls and in the host's loss pass are added to it."""
    m, n = A.shape
    states, X = [], None
    t_start = time.perf_counter()
    for i, k in enumerate(RANKS):                        # warm-up
        rows, cols = (m, n) if i == 0 else X.shape
        W_T, H = data.init_factors(seed + i, k, rows, cols)
        d = layer_call(A, X, k, W_T, H, min(10, max_iter))
        states.append([W_T, d, H])
        X = np.ascontiguousarray(H)                      # (cols, k) = t(H): the next layer's input
    total, t_loss = float("nan"), 0.0
    for _ in range(max_iter):
        X = None
        for i, k in enumerate(RANKS):
            states[i][1] = layer_call(A, X, k, states[i][0], states[i][2], 1)
            X = np.ascontiguousarray(states[i][2])
        t0 = time.perf_counter()
        total, X = 0.0, dense
        for W_T, d, H in states:                         # the reference's loss pass (fit.hpp:329-338), on the host
            R = X - (W_T * d[None, :]) @ H.T
            total += float(np.sum(R * R)) / R.size
            X = H
        t_loss += time.perf_counter() - t0
    if split is not None:
        split["host_loss_s"] = t_loss
        split["entry_calls_and_host_glue_s"] = time.perf_counter() - t_start - t_loss
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-iters", type=int, default=2)
    args = ap.parse_args()
    A = pbmc3k()
    m, n = A.shape
    dense = A.to_scipy().toarray()
    seed = 42
    r, t_res, ts_res = median_of(lambda: resident(A, args.max_iter, seed), args.reps)
    split = {}
    loss_pc, t_pc, ts_pc = median_of(lambda: per_call(A, dense, args.max_iter, seed, split), args.reps)
    rec = dict(workload="pbmc3k chain %s" % "->".join(str(k) for k in RANKS), m=m, n=n, nnz=int(A.nnz), max_iter=args.max_iter,
               solver="cholesky", precision="fp64",
               resident=dict(wall_s=t_res, runs=ts_res, iterations=r["iter"], loss=r["loss"], layer_loss=r["layer_loss"].tolist(),
                             device_op_calls_per_outer_iteration=r["counts"][0], own_kernel_launches_per_outer_iteration=r["counts"][1]),
               per_call=dict(wall_s=t_pc, runs=ts_pc, entry_calls=len(RANKS) * (args.max_iter + 1), loss=loss_pc, last_run_split=split),
               speedup=t_pc / t_res, loss_rel_diff=abs(loss_pc - r["loss"]) / abs(r["loss"]))
    if args.numpy_iters > 0:
        import factor_net_ref as F
        g = [F.layer(RANKS[0])] + [F.layer(k, "layer", [i]) for i, k in enumerate(RANKS[1:])]
        t0 = time.perf_counter()
        ref = F.fit_deep(dense, g, max_iter=args.numpy_iters, tol=0.0, seed=seed, solver=1)
        rec["numpy"] = dict(wall_s=time.perf_counter() - t0, max_iter=args.numpy_iters, loss=ref["loss"],
                            label="numpy float64 restatement (tests/factor_net_ref.py), one run, not the reference's C++")
        if args.numpy_iters == args.max_iter:
            rec["numpy"]["loss_rel_diff_resident"] = abs(ref["loss"] - r["loss"]) / abs(ref["loss"])
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
