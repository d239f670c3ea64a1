#!/usr/bin/env python3
"""tools/similarity_bench.py -- cosine() and align() on the GPU path (csrc/ops_similarity.hip).  Workload: tests/golden/pbmc3k.spz
(13 714 genes x 2 700 cells).  Three legs, each the median of --repeat (default 3) runs after one warm-up, one JSON line in all:
  cells   cosine() over the 2 700 cells (rcppml_gpu_cosine_sparse_ex, y = x): the entry end to end, its device time (from the end of
          the upload to the last kernel) and its download time
  genes   cosine() over the 13 714 genes (a 1.5 GB result): the same three figures
  align   align() of a stack of --reps (50) loadings with k = --k (10) to one reference: the dense entry and the batched match
Each leg comes with the numpy / scipy restatement of the same stage on the host (X.T @ X on scipy sparse and the norms; the dense
restatement and the restated solver for align; at most 16 threads), the launch count, and for the sparse kernel the useful
multiply-add pairs per second (work = sum over rows r of nnz_X(r) nnz_Y(r)) and the fraction of LDS tile slots touched (entries of C
that received a product / slots of all tiles).  --skip-host-genes leaves the slowest host leg out (reported as null)."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from rcppml_amd import _abi, nmf as nmf_module, similarity  # noqa: E402
from rcppml_amd.data import CSC  # noqa: E402


def pbmc3k():
    from oracle import oracle as O
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    _, m, n, _, _ = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    A = sp.csc_matrix((np.asarray(x, np.float64), np.asarray(i), np.asarray(p)), shape=(m, n))
    A.sort_indices()
    return A                                             # genes x cells


def median_of(fn, repeat):
    r = fn()                                             # warm-up
    ts, rs = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
        rs.append(r)
    return r, statistics.median(ts), rs


def sparse_leg(name, X, repeat, host):
    import similarity_ref as R
    geo = _abi.cosine_geometry()
    csc = CSC.from_scipy(X)
    out = np.empty((X.shape[1], X.shape[1]), order="F")
    r, t_total, rs = median_of(lambda: _abi.cosine_sparse(csc, out=out), repeat)
    assert r["status"] == 0, r["error"]
    dev_s = statistics.median(q["device_ms"] for q in rs) / 1e3
    down_s = statistics.median(q["download_ms"] for q in rs) / 1e3
    per_row = np.bincount(X.indices, minlength=X.shape[0]).astype(np.float64)
    work = float(np.sum(per_row * per_row))
    n = X.shape[1]
    tiles = -(-n // geo["tile"])
    touched = int(np.count_nonzero(r["C"]))
    leg = dict(columns=n, rows=X.shape[0], nnz=int(X.nnz), entry_s=t_total, device_s=dev_s, download_s=down_s,
               device_plus_download_s=dev_s + down_s, launches=r["launches"], mac_pairs=work, mac_pairs_per_s=work / dev_s,
               tile_slots_touched=touched / float(tiles * geo["tile"] * n), result_bytes=int(8 * n * n), host_s=None,
               max_abs_diff_to_host=None)
    if host:
        ref, t_ref, _ = median_of(lambda: R.cosine_sparse_ref(X), 1)
        leg.update(host_s=t_ref, max_abs_diff_to_host=float(np.max(np.abs(ref - r["C"]))))
    return {name: leg}, geo


def align_leg(A_cells, k, reps, maxit, repeat, seed):
    import similarity_ref as R
    models = [nmf_module.nmf(A_cells, k, seed=seed + i, maxit=maxit, verbose=False) for i in range(reps + 1)]
    ref, objs = models[0], models[1:]
    out, t_align, _ = median_of(lambda: similarity.align(objs, ref), repeat)
    W = np.stack([np.ascontiguousarray(np.asarray(mod.w, np.float64).T) for mod in objs])
    Rt = np.ascontiguousarray(np.asarray(ref.w, np.float64).T)
    d, t_dense, _ = median_of(lambda: _abi.cosine_dense(W, Rt, "cosine"), repeat)
    assert d["status"] == 0, d["error"]
    cost = similarity.similarity_cost(d["sim"])
    mt, t_match, _ = median_of(lambda: _abi.bipartite_match(cost), repeat)

    def host():
        sim = R.cosine_dense_ref(np.stack([np.asarray(mod.w, np.float64) for mod in objs]), np.asarray(ref.w, np.float64))
        return sim, [R.match_ref(R.similarity_cost(s))[0] for s in sim]

    (hsim, hassign), t_host, _ = median_of(host, 1)
    return dict(align=dict(reps=reps, k=k, m=int(ref.w.shape[0]), align_s=t_align, dense_entry_s=t_dense, match_host_s=t_match,
                           launches=d["launches"], host_s=t_host, max_abs_diff_to_host=float(np.max(np.abs(hsim - d["sim"]))),
                           assignments_equal_to_host=bool(np.array_equal(np.array(hassign), mt["assignment"])),
                           mean_aligned_cosine=float(np.mean([np.diag(R.cosine_dense_ref(o.w, ref.w)) for o in out]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--maxit", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--skip-host-genes", action="store_true")
    ap.add_argument("--legs", default="cells,genes,align")
    args = ap.parse_args()
    if not _abi.detect():
        raise SystemExit("similarity_bench needs a GPU")
    A = pbmc3k()
    legs = args.legs.split(",")
    out = dict(workload="pbmc3k", restatement_label="numpy / scipy restatement (tests/similarity_ref.py), not the reference's code",
               host_threads=int(os.environ["OMP_NUM_THREADS"]))
    if "cells" in legs:
        leg, geo = sparse_leg("cells", A, args.repeat, True)
        out.update(leg, geometry=geo)
    if "genes" in legs:
        G = A.T.tocsc()
        G.sort_indices()
        leg, geo = sparse_leg("genes", G, args.repeat, not args.skip_host_genes)
        out.update(leg, geometry=geo)
    if "align" in legs:
        cells_rows = A.T.tocsc()
        out.update(align_leg(cells_rows, args.k, args.reps, args.maxit, args.repeat, args.seed))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
